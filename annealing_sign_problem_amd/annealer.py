"""The ``ising_glass_annealer`` surface the reference uses (``import
ising_glass_annealer as sa``; annealing_sign_problem/common.py:8), served by the
gfx950 sweep kernel through the C ABI:

    sa.Hamiltonian(exchange, field)      common.py:204,681
    sa.anneal(h, seed=, number_sweeps=, repetitions=, only_best=)
                                         common.py:242-248,
                                         experiments/full_hilbert_space.py:212-218
    sa.anneal(h, x0, seed=, number_sweeps=, beta0=, beta1=)   (legacy keywords)
                                         annealing_sign_problem/train.py:238-245,297
    sa.signs_to_bits / sa.bits_to_signs  common.py:205,224-225,258-260
    sa.greedy_solve(h)                   common.py:250

Conventions pinned by the reference: the solver MINIMISES
``E(s) = sum_ij J_ij s_i s_j + sum_i h_i s_i`` (full double sum, diagonal
included, no 1/2: common.py:757-760, experiments/full_hilbert_space.py:142-145);
bit ``i`` of word ``i // 64`` is set iff ``s_i = +1`` (cbits/build_matrix.c:72-74).
The annealing schedule, RNG and sweep order are this package's own
specification: the reference's annealer is a third-party library
whose internals are not available.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np
import scipy.sparse

from . import _lib

__all__ = [
    "Hamiltonian",
    "PatternMismatch",
    "reweight_hamiltonians",
    "plan_hamiltonians",
    "plan_hamiltonians_last_ms",
    "read_plan_array",
    "anneal",
    "anneal_batch",
    "anneal_traces",
    "anneal_until",
    "Chains",
    "resample_chains",
    "population_anneal",
    "population_anneal_batch",
    "parallel_tempering",
    "parallel_tempering_batch",
    "parallel_tempering_cluster",
    "parallel_tempering_cluster_batch",
    "advance_ladder_chains",
    "exchange_chains",
    "cluster_move_chains",
    "consensus_chains",
    "greedy_solve",
    "greedy_solve_batch",
    "signs_to_bits",
    "bits_to_signs",
    "make_schedule",
]


def signs_to_bits(signs) -> np.ndarray:
    """Pack a ±1 array: bit i of word i // 64 is set iff ``signs[i] > 0``."""
    signs = np.asarray(signs)
    n = signs.shape[0]
    positive = (signs > 0).astype(np.uint8)
    padded = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    padded[:n] = positive
    return np.packbits(padded.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def bits_to_signs(bits, count: int) -> np.ndarray:
    """Unpack ``count`` spins to a float64 array of ±1."""
    bits = np.ascontiguousarray(bits, dtype="<u8").reshape(-1)
    count = int(count)
    if count > bits.shape[0] * 64:
        raise ValueError("'bits' holds fewer than {} spins".format(count))
    unpacked = np.unpackbits(bits.view(np.uint8), bitorder="little")[:count]
    return 2.0 * unpacked.astype(np.float64) - 1.0


def make_schedule(beta0: float, beta1: float, number_sweeps: int) -> np.ndarray:
    """Geometric inverse-temperature ladder beta0 -> beta1, one value per sweep."""
    number_sweeps = int(number_sweeps)
    if number_sweeps <= 0:
        return np.zeros(0, dtype=np.float64)
    if not (beta0 > 0 and beta1 > 0 and np.isfinite(beta0) and np.isfinite(beta1)):
        raise ValueError("beta0 and beta1 must be positive and finite")
    if number_sweeps == 1:
        return np.array([beta1], dtype=np.float64)
    return np.geomspace(beta0, beta1, number_sweeps).astype(np.float64)


class PatternMismatch(ValueError):
    """:meth:`Hamiltonian.reweight` was given couplings on another sparsity pattern than the plan's
    (or numbers under which ``J + J^T`` gains or loses an entry): the plan cannot take them."""


class Hamiltonian:
    """Classical Ising Hamiltonian ``E(s) = s^T J s + h^T s`` resident on the GPU.

    ``exchange`` may be any scipy sparse matrix (the reference hands over COO,
    common.py:196,204); it is stored as canonical CSR so that the reference's
    later ``.tocoo()``, ``.tocsr()`` and ``[mask][:, mask]`` uses work
    (common.py:444,654,674).
    """

    def __init__(self, exchange, field):
        matrix = scipy.sparse.csr_matrix(exchange, dtype=np.float64, copy=True)  # (frozen below)
        if matrix.shape[0] != matrix.shape[1]:
            raise ValueError("'exchange' must be square, got {}".format(matrix.shape))
        matrix.sum_duplicates()
        matrix.sort_indices()
        field = np.array(field, dtype=np.float64, order="C", copy=True)
        if field.shape != (matrix.shape[0],):
            raise ValueError("'field' must have shape ({},)".format(matrix.shape[0]))
        # The device plan is built once from these arrays and cached (the key is the identity of
        # the two objects): they are frozen, so an in-place edit raises instead of leaving a stale
        # plan behind.  Assigning a NEW matrix or field to the attributes rebuilds the plan.
        for array in (matrix.data, matrix.indices, matrix.indptr, field):
            array.flags.writeable = False
        self.exchange = matrix
        self.field = field
        self._plan = None
        self._plan_key = None

    @classmethod
    def from_canonical_csr(cls, indptr, indices, data, field) -> "Hamiltonian":
        """A Hamiltonian from CSR arrays that ARE canonical already — rows in order, columns
        sorted and duplicate-free, as the device builders deliver them (asp_operator_ising,
        asp_sparsify_component) — without the copy, ``sum_duplicates`` and ``sort_indices`` of the
        general constructor (a quarter of the host time of a sampled-cluster run went there).  The
        arrays are adopted and frozen; ``asp_sa_plan_create`` still validates them."""
        indptr = np.ascontiguousarray(indptr)
        n = indptr.shape[0] - 1
        matrix = scipy.sparse.csr_matrix((np.ascontiguousarray(data, dtype=np.float64),
                                          np.ascontiguousarray(indices), indptr), shape=(n, n), copy=False)
        matrix.has_sorted_indices = True
        matrix.has_canonical_format = True
        field = np.ascontiguousarray(field, dtype=np.float64)
        if field.shape != (n,):
            raise ValueError("'field' must have shape ({},)".format(n))
        self = cls.__new__(cls)
        for array in (matrix.data, matrix.indices, matrix.indptr, field):
            array.flags.writeable = False
        self.exchange = matrix
        self.field = field
        self._plan = None
        self._plan_key = None
        return self

    @property
    def shape(self) -> Tuple[int, int]:
        return self.exchange.shape

    @property
    def size(self) -> int:
        return self.exchange.shape[0]

    # -- device plan -----------------------------------------------------------
    def _arrays(self):
        m = self.exchange
        return (
            np.ascontiguousarray(m.indptr, dtype=np.int64),
            np.ascontiguousarray(m.indices, dtype=np.int32),
            np.ascontiguousarray(m.data, dtype=np.float64),
            np.ascontiguousarray(self.field, dtype=np.float64),
        )

    def plan(self):
        """The (cached) device-resident sweep plan handle."""
        key = self._key()
        if self._plan is not None and self._plan_key == key:
            return self._plan
        self._release_plan()
        lib = _lib.load()
        _lib.require_gpu()
        indptr, indices, data, field = self._arrays()
        handle = lib.asp_sa_plan_create(ctypes.c_uint64(self.size), _lib.ptr(indptr),
                                        _lib.ptr(indices), _lib.ptr(data), _lib.ptr(field))
        if not handle:
            raise _lib.AspError(lib.asp_last_error_code(), _lib.last_error())
        self._plan = ctypes.c_void_p(handle)
        self._plan_key = key
        _lib.track(self)
        return self._plan

    def info(self) -> _lib.SaInfo:
        info = _lib.SaInfo()
        _lib.check(_lib.load().asp_sa_plan_info(self.plan(), ctypes.byref(info)))
        return info

    def release(self) -> None:
        """Destroy the device plan now (it is rebuilt on the next use), and the coupling stencil of the
        family when this Hamiltonian is the one it was made for."""
        family = getattr(self, "_family", None)
        if family and family.get("owner") == id(self):
            stencil = family.pop("stencil", None)
            family.pop("owner", None)
            family.pop("pattern", None)
            if stencil:
                stencil.release()
        self._release_plan()

    def _release_plan(self) -> None:
        if self._plan is not None:
            try:
                _lib.load().asp_sa_plan_destroy(self._plan)
            finally:
                self._plan = None
                self._plan_key = None

    def __del__(self):
        # never reach into HIP from interpreter teardown: _lib.shutdown (atexit) has released
        # every live plan before that point
        if getattr(self, "_plan", None) is None or _lib.closed():
            return
        try:
            self.release()
        except Exception:
            pass

    # -- new numbers on the same pattern ------------------------------------------
    def _key(self):
        return (id(self.exchange), id(self.field), self.exchange.nnz)

    def reweight(self, data, field=None, indptr=None, indices=None) -> "Hamiltonian":
        """New couplings ``data`` (in the order of ``exchange.data``; ``None`` keeps them) and / or a
        new ``field`` on the SAME sparsity pattern, in place: the device plan takes the numbers without
        being rebuilt (``asp_sa_plan_reweight``: no colouring, no permutation, no ELL fill) and
        afterwards equals, bit for bit, the plan of ``Hamiltonian(new exchange, new field)``.
        ``indptr`` / ``indices``, when given, are compared with the pattern; any difference — and
        numbers under which ``J + J^T`` gains or loses an entry — raises :class:`PatternMismatch`
        and leaves the object as it was.  Live :class:`Chains` of this object must be closed first.
        ``exchange`` and ``field`` become new frozen objects that share the frozen index arrays."""
        m = self.exchange
        if indptr is not None and not np.array_equal(np.asarray(indptr), m.indptr):
            raise PatternMismatch("'indptr' differs from the pattern of this Hamiltonian")
        if indices is not None and not np.array_equal(np.asarray(indices), m.indices):
            raise PatternMismatch("'indices' differ from the pattern of this Hamiltonian")
        if data is None and field is None:
            raise ValueError("at least one of 'data' and 'field' must be given")
        if data is not None:
            data = np.array(data, dtype=np.float64, order="C", copy=True).reshape(-1)
            if data.shape[0] != m.nnz:
                raise PatternMismatch("{} couplings given, the pattern has {}".format(data.shape[0], m.nnz))
        if field is not None:
            field = np.array(field, dtype=np.float64, order="C", copy=True)
            if field.shape != (self.size,):
                raise ValueError("'field' must have shape ({},)".format(self.size))
        plan = self.plan()
        old_indptr, old_indices, _, _ = self._arrays()
        lib = _lib.load()
        rc = lib.asp_sa_plan_reweight(plan, ctypes.c_uint64(m.nnz), _lib.ptr(old_indptr), _lib.ptr(old_indices),
                                      _lib.ptr(data), _lib.ptr(field))
        if rc != 0:
            message = _lib.last_error()
            if "pattern mismatch" in message:
                raise PatternMismatch(message)
            raise _lib.AspError(rc, message)
        if data is not None:
            data.flags.writeable = False  # (before scipy takes its view of it)
            matrix = scipy.sparse.csr_matrix((data, m.indices, m.indptr), shape=m.shape, copy=False)
            matrix.has_sorted_indices = True
            matrix.has_canonical_format = True
            self.exchange = matrix
        if field is not None:
            field.flags.writeable = False
            self.field = field
        self._plan_key = self._key()
        return self

    def clone(self) -> "Hamiltonian":
        """A NEW Hamiltonian with the numbers and the structure of this one (which gets its plan built if
        it has none): its plan is a clone of this one's (``asp_sa_plan_clone``: own buffers and stream, no
        preprocessing).  It belongs to this one's family (:meth:`family`)."""
        source = self.plan()
        lib = _lib.load()
        handle = ctypes.c_void_p()
        _lib.check(lib.asp_sa_plan_clone(source, ctypes.byref(handle)))
        other = Hamiltonian.__new__(Hamiltonian)
        other.exchange = self.exchange
        other.field = self.field
        other._plan = handle
        other._plan_key = other._key()
        other._family = self.family()
        _lib.track(other)
        return other

    def family(self) -> dict:
        """What a Hamiltonian and its clones share besides the pattern: a dict that
        ``common.reweight_ising_models`` keeps the coupling stencil in (``"stencil"``, with ``"owner"``,
        the ``id`` of the Hamiltonian whose :meth:`release` closes it)."""
        family = getattr(self, "_family", None)
        if family is None:
            family = self._family = {}
        return family

    def reweighted(self, data, field=None, indptr=None, indices=None) -> "Hamiltonian":
        """A NEW Hamiltonian with these numbers on the pattern of this one (which is left alone and
        gets its plan built if it has none): its plan is a clone of this one's (``asp_sa_plan_clone``:
        the same structure, own buffers and stream, no preprocessing) reweighted as in
        :meth:`reweight`.  The two objects can go into one batched call."""
        other = self.clone()
        try:
            other.reweight(data, field, indptr, indices)
        except Exception:
            other.release()
            raise
        return other

    # -- energy ----------------------------------------------------------------
    def energy(self, x) -> float:
        """E(x) of one packed configuration (experiments/full_hilbert_space.py:144)."""
        return float(self.energies(np.asarray(x).reshape(1, -1))[0])

    def energies(self, xs) -> np.ndarray:
        words = (self.size + 63) // 64
        xs = np.ascontiguousarray(xs, dtype=np.uint64).reshape(-1, max(words, 1))
        if xs.shape[1] != max(words, 1):
            raise ValueError("configurations must have {} words".format(words))
        out = np.zeros(xs.shape[0], dtype=np.float64)
        _lib.check(_lib.load().asp_sa_energy(self.plan(), ctypes.c_uint32(xs.shape[0]),
                                             _lib.ptr(xs), _lib.ptr(out)))
        return out


def reweight_hamiltonians(hamiltonians, stencil, psis, fields=None) -> list:
    """:meth:`Hamiltonian.reweight` of many Hamiltonians of ONE pattern in one device call
    (``asp_sa_plan_reweight_stencil_batch``): Hamiltonian ``d`` takes the couplings
    that ``stencil`` (``operators.IsingStencil`` of that pattern) forms from the amplitudes ``psis[d]``
    — they never visit the host on their way into the plan — and, with ``fields``, the field
    ``fields[d]`` (``None``: kept).  In place; returns one bool per Hamiltonian.  ``True``: applied,
    ``exchange.data`` and ``field`` hold the new numbers (new frozen objects that share the frozen index
    arrays).  ``False``: that draw's couplings leave the pattern, the Hamiltonian is untouched.  The
    Hamiltonians must be distinct objects with distinct plans and no live :class:`Chains`; any refusal
    (``AspError`` with the item's index in the message) leaves all of them as they were."""
    hamiltonians = list(hamiltonians)
    count = len(hamiltonians)
    psis = np.ascontiguousarray(psis, dtype=np.float64)
    if psis.ndim != 2 or psis.shape[0] != count:
        raise ValueError("'psis' should hold one row of amplitudes per Hamiltonian")
    if fields is not None:
        fields = np.ascontiguousarray(fields, dtype=np.float64)
        if fields.shape != psis.shape:
            raise ValueError("'fields' should have the shape of 'psis'")
    for h in hamiltonians:
        if h.size != psis.shape[1]:
            raise ValueError("'psis' should hold {} amplitudes per row".format(h.size))
    handle = stencil.handle()
    if count == 0:
        return []
    lib = _lib.load()
    items = (_lib.SaStencilItem * count)()
    data = [np.empty(stencil.nnz, dtype=np.float64) for _ in range(count)]  # (each adopted by its exchange)
    for d, h in enumerate(hamiltonians):
        items[d].plan = h.plan()
        items[d].psi = psis[d].ctypes.data
        items[d].field = None if fields is None else fields[d].ctypes.data
        items[d].data_out = data[d].ctypes.data
        items[d].status = 0
    _lib.check(lib.asp_sa_plan_reweight_stencil_batch(handle, items, ctypes.c_uint32(count)))
    applied = []
    for d, h in enumerate(hamiltonians):
        applied.append(items[d].status == 0)
        if not applied[-1]:
            continue
        m = h.exchange
        values = data[d]
        values.flags.writeable = False  # (before scipy takes its view of it)
        matrix = scipy.sparse.csr_matrix((values, m.indices, m.indptr), shape=m.shape, copy=False)
        matrix.has_sorted_indices = True
        matrix.has_canonical_format = True
        h.exchange = matrix
        if fields is not None:
            field = fields[d].copy()
            field.flags.writeable = False
            h.field = field
        h._plan_key = h._key()
    return applied


def reweight_hamiltonians_last_ms() -> float:
    """Device time (ms, HIP events) of this thread's last :func:`reweight_hamiltonians`."""
    return float(_lib.load().asp_sa_plan_reweight_stencil_last_ms())


PLAN_ARRAYS = {  # asp_sa_plan_read_array: name -> (id, dtype)
    "color_block_start": (0, np.uint32), "block_width": (1, np.uint32), "ell_off": (2, np.uint64),
    "ell_col": (3, np.uint32), "ell_col4": (4, np.uint32), "ell_val": (5, np.float64),
    "spin_of_pos": (6, np.uint32), "pos_of_spin": (7, np.uint32), "field_pos": (8, np.float64),
}


def read_plan_array(plan, name: str) -> np.ndarray:
    """The device array ``name`` (a key of ``PLAN_ARRAYS``) of a plan handle, copied to the host; an
    empty array where the plan does not hold it (``asp_sa_plan_read_array``)."""
    which, dtype = PLAN_ARRAYS[name]
    lib = _lib.load()
    size = ctypes.c_uint64(0)
    rc = lib.asp_sa_plan_read_array(plan, which, None, ctypes.c_uint64(0), ctypes.byref(size))
    if size.value == 0:
        _lib.check(rc)
        return np.empty(0, dtype=dtype)
    out = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
    _lib.check(lib.asp_sa_plan_read_array(plan, which, _lib.ptr(out), ctypes.c_uint64(out.nbytes),
                                          ctypes.byref(size)))
    return out


def plan_hamiltonians(hamiltonians) -> None:
    """:meth:`Hamiltonian.plan` of many Hamiltonians in ONE device call (``asp_sa_plan_create_segments``,
    DESIGN.md §4.15): every Hamiltonian without a valid cached plan gets the plan its own ``plan()`` would
    have made, bit for bit; those with one are left alone.  A refusal (``AspError``, the message naming
    the first offending Hamiltonian as "segment g" among the ones that were planned) leaves all of them
    without a plan."""
    todo, seen = [], set()
    for h in hamiltonians:
        if id(h) in seen or (h._plan is not None and h._plan_key == h._key()):
            continue
        seen.add(id(h))
        todo.append(h)
    if not todo:
        return
    lib = _lib.load()
    _lib.require_gpu()
    for h in todo:
        h._release_plan()  # (a stale one)
    arrays = [h._arrays() for h in todo]
    offsets = np.zeros(len(todo) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([h.size for h in todo], dtype=np.uint64)
    entries = np.zeros(len(todo) + 1, dtype=np.int64)
    entries[1:] = np.cumsum([a[1].size for a in arrays], dtype=np.int64)
    indptr = np.zeros(int(offsets[-1]) + 1, dtype=np.int64)
    for g, a in enumerate(arrays):
        indptr[int(offsets[g]) + 1:int(offsets[g + 1]) + 1] = a[0][1:] + entries[g]
    indices = np.concatenate([a[1] for a in arrays]) if arrays else np.empty(0, dtype=np.int32)
    data = np.concatenate([a[2] for a in arrays])
    field = np.concatenate([a[3] for a in arrays])
    plans = (ctypes.c_void_p * len(todo))()
    _lib.check(lib.asp_sa_plan_create_segments(ctypes.c_uint64(len(todo)), _lib.ptr(offsets), _lib.ptr(indptr),
                                               _lib.ptr(np.ascontiguousarray(indices, dtype=np.int32)),
                                               _lib.ptr(np.ascontiguousarray(data, dtype=np.float64)),
                                               _lib.ptr(np.ascontiguousarray(field, dtype=np.float64)), plans))
    for h, handle in zip(todo, plans):
        h._plan = ctypes.c_void_p(handle)
        h._plan_key = h._key()
        _lib.track(h)


def plan_hamiltonians_last_ms() -> float:
    """Device time (ms, HIP events; copies excluded) of this thread's last :func:`plan_hamiltonians`
    call that had anything to plan."""
    return float(_lib.load().asp_sa_plan_segments_last_ms())


def resolve_sweep_order(sweep_order: Optional[str]) -> str:
    """``"shuffled"`` or ``"colour"``; ``None`` reads ``$ASP_SWEEP_ORDER`` and falls back to
    ``"shuffled"`` — the visiting order of the reference's annealer, so
    that every drop-in entry point (``sa.anneal``, ``common.solve_ising_model``, `make small`,
    ``sampled_components --annealing``) runs the chain with the reference's law unless told
    otherwise.  ``"colour"`` (ASP-SA-1's fixed order: faster here, a different Markov chain) is
    one keyword / flag / environment variable away."""
    if sweep_order is None:
        sweep_order = os.environ.get("ASP_SWEEP_ORDER") or "shuffled"
    if sweep_order not in ("colour", "shuffled"):
        raise ValueError("'sweep_order' must be 'colour' or 'shuffled'")
    return sweep_order


def _resolve_seed(seed) -> int:
    if seed is None:
        return int.from_bytes(os.urandom(8), "little")
    return int(seed) & (2**64 - 1)


def anneal_raw(hamiltonian: Hamiltonian, seed: int, betas: np.ndarray, repetitions: int,
               replica_offset: int = 0, x0=None, shuffled: bool = False):
    """All chains, no reduction: (xs[R, words] uint64, es[R] float64).  ``shuffled``: a fresh
    visiting order every sweep (``asp_sa_anneal_shuffled``) instead of the colour order."""
    lib = _lib.load()
    plan = hamiltonian.plan()
    words = (hamiltonian.size + 63) // 64
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    xs = np.zeros((repetitions, max(words, 1)), dtype=np.uint64)
    es = np.zeros(repetitions, dtype=np.float64)
    if x0 is not None:
        x0 = np.ascontiguousarray(x0, dtype=np.uint64).reshape(-1)
        if x0.shape[0] != words:
            raise ValueError("'x0' must have {} words".format(words))
    entry = lib.asp_sa_anneal_shuffled if shuffled else lib.asp_sa_anneal
    _lib.check(entry(plan, ctypes.c_uint64(seed), _lib.ptr(betas),
                     ctypes.c_uint32(betas.shape[0]), ctypes.c_uint32(repetitions),
                     ctypes.c_uint32(replica_offset), _lib.ptr(x0), _lib.ptr(xs), _lib.ptr(es)))
    return xs[:, :words], es


def set_tail(hamiltonian: Hamiltonian, n: int = -1) -> None:
    """``asp_sa_set_tail``: -1 automatic, 0 no tail sweeps, n > 0 tail sweeps below n flips per sweep."""
    _lib.check(_lib.load().asp_sa_set_tail(hamiltonian.plan(), int(n)))


def last_tail(hamiltonian: Hamiltonian):
    """``asp_sa_last_tail`` of the last closed colour call: (sweeps_min, sweeps_max, entries_max)."""
    out = [ctypes.c_uint32(0) for _ in range(3)]
    _lib.check(_lib.load().asp_sa_last_tail(hamiltonian.plan(), *[ctypes.byref(v) for v in out]))
    return tuple(int(v.value) for v in out)


def anneal_raw_into(hamiltonian: Hamiltonian, seed: int, betas: np.ndarray, repetitions: int,
                    replica_offset: int, x0, out_x_ptr: int, out_e_ptr: int,
                    shuffled: bool = False) -> None:
    """``anneal_raw`` writing into caller-owned memory given as raw addresses — host or DEVICE
    (e.g. ``tensor.data_ptr()`` of torch tensors on this library's GPU): ``out_x`` receives
    ``repetitions * ceil(K/64)`` words, ``out_e`` ``repetitions`` doubles."""
    lib = _lib.load()
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    if x0 is not None:
        x0 = np.ascontiguousarray(x0, dtype=np.uint64).reshape(-1)
        if x0.shape[0] != (hamiltonian.size + 63) // 64:
            raise ValueError("'x0' must have {} words".format((hamiltonian.size + 63) // 64))
    entry = lib.asp_sa_anneal_shuffled if shuffled else lib.asp_sa_anneal
    _lib.check(entry(hamiltonian.plan(), ctypes.c_uint64(seed), _lib.ptr(betas),
                     ctypes.c_uint32(betas.shape[0]), ctypes.c_uint32(repetitions),
                     ctypes.c_uint32(replica_offset), _lib.ptr(x0),
                     ctypes.c_void_p(out_x_ptr), ctypes.c_void_p(out_e_ptr)))


def anneal(hamiltonian: Hamiltonian, x0=None, seed=None, number_sweeps: int = 5120,
           beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 1,
           only_best: bool = True, distributed: bool = True, sweep_order: Optional[str] = None):
    """Simulated annealing of ``hamiltonian``.

    Returns ``(x, e)``: with ``only_best=True`` the best packed configuration
    (``uint64[ceil(K/64)]``) over all repetitions and its energy; with
    ``only_best=False`` the per-repetition arrays ``(xs[R, words], es[R])``
    (zip-able, experiments/full_hilbert_space.py:176).

    ``sweep_order="shuffled"`` (default): a fresh random visiting order every sweep — what the
    reference's ``ising_glass_annealer`` does as far as its published success probabilities can
    tell: statistically the library's behaviour.
    ``sweep_order="colour"``: the fixed colour order of specification ASP-SA-1 — a different
    Markov chain (a HIGHER success probability per sweep than the published curves) and several
    times the rate on this hardware; the headline kernel of ``bench.py``.  ``None``: the value of
    ``$ASP_SWEEP_ORDER`` if set, else ``"shuffled"``.

    When ``torch.distributed`` is initialised with more than one rank (and
    ``distributed`` is true) the repetitions are sharded over the ranks and
    gathered at the end (see :mod:`.distributed`); every rank returns the full
    result, identical to a single-GPU run with the same seed.
    """
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    from . import distributed as _dist  # late import: torch is optional plumbing

    shuffled = resolve_sweep_order(sweep_order) == "shuffled"
    sharded = distributed and _dist.shards_chains()
    seed = _dist.agree_on_seed(seed) if sharded else _resolve_seed(seed)
    if beta0 is None or beta1 is None:
        info = hamiltonian.info()
        beta0 = info.beta0_auto if beta0 is None else beta0
        beta1 = info.beta1_auto if beta1 is None else beta1
    betas = make_schedule(float(beta0), float(beta1), number_sweeps)

    if sharded and only_best:
        return _dist.anneal_sharded_best(hamiltonian, seed, betas, repetitions, x0, shuffled=shuffled)
    if sharded:
        xs, es = _dist.anneal_sharded(hamiltonian, seed, betas, repetitions, x0, shuffled=shuffled)
    else:
        xs, es = anneal_raw(hamiltonian, seed, betas, repetitions, 0, x0, shuffled=shuffled)
    if only_best:
        best = int(np.argmin(es))  # first minimum: deterministic tie-break
        return xs[best].copy(), float(es[best])
    return xs, es


def anneal_batch_raw(hamiltonians, seeds, schedules, repetitions, replica_offsets=None,
                     shuffled: bool = False):
    """Many independent problems in ONE device call (``asp_sa_anneal_batch``): problem ``i`` is
    ``anneal_raw(hamiltonians[i], seeds[i], schedules[i], repetitions[i], replica_offsets[i])``,
    chain for chain, but the groups of all problems share a few launches, so a batch of small
    clusters fills the chip.  ``shuffled``: every problem is an ``asp_sa_anneal_shuffled`` call
    (a fresh visiting order every sweep); their kernels overlap on the problems' own streams.
    Returns ``[(xs, es), ...]`` in order."""
    lib = _lib.load()
    n = len(hamiltonians)
    repetitions = [int(r) for r in (repetitions if np.ndim(repetitions) else [repetitions] * n)]
    offsets = [0] * n if replica_offsets is None else [int(o) for o in replica_offsets]
    if not (len(seeds) == len(schedules) == len(repetitions) == len(offsets) == n):
        raise ValueError("anneal_batch_raw: argument lengths differ")
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("anneal_batch_raw: every problem needs its own Hamiltonian object")
    items = (_lib.SaBatchItem * max(n, 1))()
    keep, out = [], []
    for i, h in enumerate(hamiltonians):
        words = (h.size + 63) // 64
        betas = np.ascontiguousarray(schedules[i], dtype=np.float64)
        xs = np.zeros((repetitions[i], max(words, 1)), dtype=np.uint64)
        es = np.zeros(repetitions[i], dtype=np.float64)
        keep.append(betas)
        out.append((xs, es, words))
        items[i].plan = h.plan()
        items[i].seed = int(seeds[i]) & (2**64 - 1)
        items[i].betas = betas.ctypes.data
        items[i].num_sweeps = betas.shape[0]
        items[i].repetitions = repetitions[i]
        items[i].replica_offset = offsets[i]
        items[i].flags = _lib.SA_BATCH_SHUFFLED if shuffled else 0
        items[i].out_x = xs.ctypes.data
        items[i].out_e = es.ctypes.data
    _lib.check(lib.asp_sa_anneal_batch(items, ctypes.c_uint32(n)))
    return [(xs[:, :words], es) for xs, es, words in out]


def anneal_batch(hamiltonians, seed=None, number_sweeps: int = 5120, repetitions: int = 64,
                 only_best: bool = True, beta0: Optional[float] = None,
                 beta1: Optional[float] = None, sweep_order: Optional[str] = None):
    """``[anneal(h, seed=seed, number_sweeps=..., repetitions=..., only_best=...) for h in
    hamiltonians]`` in one device call — identical results (each problem keeps its own automatic
    ladder and the same chains), a fraction of the time for many small problems.  ``seed`` may be
    one value for all problems (what the reference's per-cluster loop passes, common.py:236) or
    a sequence.  Chains stay on this rank (cluster instances are what shards over ranks)."""
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    for h in hamiltonians:
        if not isinstance(h, Hamiltonian):
            raise TypeError("'hamiltonians' must hold Hamiltonian objects")
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    if seed is None or np.ndim(seed) == 0:
        seeds = [_resolve_seed(seed) for _ in range(n)] if seed is None else [_resolve_seed(seed)] * n
    else:
        seeds = [_resolve_seed(x) for x in seed]
    schedules = []
    for h in hamiltonians:
        b0, b1 = beta0, beta1
        if b0 is None or b1 is None:
            info = h.info()
            b0 = info.beta0_auto if b0 is None else b0
            b1 = info.beta1_auto if b1 is None else b1
        schedules.append(make_schedule(float(b0), float(b1), number_sweeps))
    results = anneal_batch_raw(hamiltonians, seeds, schedules, [repetitions] * n,
                               shuffled=resolve_sweep_order(sweep_order) == "shuffled")
    if not only_best:
        return results
    best = []
    for xs, es in results:
        k = int(np.argmin(es))  # first minimum, as anneal()
        best.append((xs[k].copy(), float(es[k])))
    return best


def anneal_trace_raw(hamiltonian: Hamiltonian, seed: int, betas: np.ndarray, repetitions: int,
                     replica_offset: int = 0, x0=None, shuffled: bool = False):
    """``anneal_raw`` plus ``trace int64[R, T+1]``: tracked energy of every chain after each
    sweep in units of ``2**-energy_scale_exp``, relative to its initial configuration.
    ``shuffled``: a fresh visiting order every sweep (``asp_sa_anneal_shuffled_trace``) instead of
    the colour order (``asp_sa_anneal_trace``), as in ``anneal_raw``."""
    lib = _lib.load()
    plan = hamiltonian.plan()
    words = (hamiltonian.size + 63) // 64
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    xs = np.zeros((repetitions, max(words, 1)), dtype=np.uint64)
    es = np.zeros(repetitions, dtype=np.float64)
    trace = np.zeros((repetitions, betas.shape[0] + 1), dtype=np.int64)
    if x0 is not None:
        x0 = np.ascontiguousarray(x0, dtype=np.uint64).reshape(-1)
        if x0.shape[0] != words:
            raise ValueError("'x0' must have {} words".format(words))
    entry = lib.asp_sa_anneal_shuffled_trace if shuffled else lib.asp_sa_anneal_trace
    _lib.check(entry(plan, ctypes.c_uint64(seed), _lib.ptr(betas),
                     ctypes.c_uint32(betas.shape[0]), ctypes.c_uint32(repetitions),
                     ctypes.c_uint32(replica_offset), _lib.ptr(x0),
                     _lib.ptr(xs), _lib.ptr(es), _lib.ptr(trace)))
    return xs[:, :words], es, trace


def anneal_traces(hamiltonian: Hamiltonian, x0=None, seed=None, number_sweeps: int = 5120,
                  beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 1,
                  sweep_order: Optional[str] = None):
    """``anneal(..., only_best=False)`` with the energy of every chain after every sweep:
    ``(xs[R, words], es[R], e_current[R, T+1], e_best[R, T+1])`` in energy units.  Column 0 is the
    initial configuration, ``e_best`` the running minimum of ``e_current``, ``e_best[r, -1] ==
    es[r]``.

    Every chain is anchored the way ``anneal_with_traces`` anchors its one chain: the traces are
    the kernel's exact integer bookkeeping of the accepted ``dE``, shifted so that the chain's best
    value is ``es[r]``, the returned configuration's energy recomputed in full precision.

    ``sweep_order`` as in ``anneal``: ``None`` (default) is ``$ASP_SWEEP_ORDER`` if set, else
    ``"shuffled"`` — the chains ``anneal`` runs with the same seed.  Chains stay on this rank."""
    shuffled = resolve_sweep_order(sweep_order) == "shuffled"  # (first: a bad order fails without a GPU)
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    info = hamiltonian.info()
    beta0 = info.beta0_auto if beta0 is None else beta0
    beta1 = info.beta1_auto if beta1 is None else beta1
    betas = make_schedule(float(beta0), float(beta1), number_sweeps)
    xs, es, trace = anneal_trace_raw(hamiltonian, _resolve_seed(seed), betas, repetitions, 0, x0,
                                     shuffled=shuffled)
    unit = 2.0 ** -info.energy_scale_exp
    best = np.minimum.accumulate(trace, axis=1)
    floor = best[:, -1:]
    e_best = es[:, None] + (best - floor).astype(np.float64) * unit
    e_current = es[:, None] + (trace - floor).astype(np.float64) * unit
    return xs, es, e_current, e_best


class Chains:
    """Resumable annealing chains of ``hamiltonian`` on the device (``asp_sa_chains``, DESIGN.md
    §4.10): ``repetitions`` chains that are advanced a segment of sweeps at a time, looked at,
    checkpointed and continued.  Any split of a schedule into ``advance`` calls gives exactly the
    chains of the closed call (``anneal_raw`` with the same seed, ``x0`` and ``replica_offset``).

    ``x0``: ``None`` (the random start of ``anneal``), one packed configuration ``[words]`` shared
    by every chain, or ``[repetitions, words]`` with a start of its own for every chain."""

    _ORDERS = {"colour": 0, "shuffled": 1}

    def __init__(self, hamiltonian: Hamiltonian, seed=None, repetitions: int = 1, x0=None,
                 replica_offset: int = 0):
        if not isinstance(hamiltonian, Hamiltonian):
            raise TypeError("'hamiltonian' must be a Hamiltonian")
        repetitions = int(repetitions)
        if repetitions < 1:
            raise ValueError("'repetitions' must be positive")
        self._handle = None
        self.hamiltonian = hamiltonian
        self.repetitions = repetitions
        self.replica_offset = int(replica_offset)
        self.seed = _resolve_seed(seed)
        self.words = (hamiltonian.size + 63) // 64
        stride = 0
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.uint64)
            if x0.ndim == 1:
                if x0.shape[0] != self.words:
                    raise ValueError("a shared 'x0' must have {} words".format(self.words))
            elif x0.ndim == 2:
                if x0.shape != (repetitions, self.words):
                    raise ValueError("a per-chain 'x0' must have shape ({}, {})".format(repetitions, self.words))
                stride = self.words
                if self.words == 0:
                    x0 = None
            else:
                raise ValueError("'x0' must be a packed configuration [words] or one per chain [repetitions, words]")
        lib = _lib.load()
        self._plan = hamiltonian.plan()
        handle = ctypes.c_void_p()
        _lib.check(lib.asp_sa_chains_create(self._plan, ctypes.c_uint64(self.seed), ctypes.c_uint32(repetitions),
                                            ctypes.c_uint32(self.replica_offset), _lib.ptr(x0),
                                            ctypes.c_uint64(stride), ctypes.byref(handle)))
        self._handle = handle
        _lib.track(self)

    def _live(self):
        if self._handle is None:
            raise ValueError("these chains are closed")
        if self.hamiltonian._plan is None or self.hamiltonian._plan.value != self._plan.value:
            raise ValueError("the Hamiltonian's device plan was released or rebuilt: these chains are gone with it")
        return self._handle

    @property
    def sweeps_done(self) -> int:
        return int(self._export([])["sweeps_done"])  # (no arrays: the counter only, no device work)

    def advance(self, betas, sweep_order: Optional[str] = None, trace: bool = False):
        """Run ``len(betas)`` more sweeps, sweep ``k`` at inverse temperature ``betas[k]``.
        ``sweep_order`` as in ``anneal`` (``None``: ``$ASP_SWEEP_ORDER``, else ``"shuffled"``); it may
        differ from segment to segment.  ``trace=True`` returns ``int64[R, len(betas) + 1]``: the
        tracked energy before the segment and after each of its sweeps, in units of
        ``2**-energy_scale_exp`` relative to the chain's very first configuration; else ``None``."""
        order = self._ORDERS[resolve_sweep_order(sweep_order)]
        handle = self._live()
        betas = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        rows = np.zeros((self.repetitions, betas.shape[0] + 1), dtype=np.int64) if trace else None
        _lib.check(_lib.load().asp_sa_chains_advance(handle, _lib.ptr(betas), ctypes.c_uint32(betas.shape[0]),
                                                     ctypes.c_uint32(order), _lib.ptr(rows)))
        return rows

    def _chain_betas(self, chain_betas) -> np.ndarray:
        chain_betas = np.ascontiguousarray(chain_betas, dtype=np.float64)
        if chain_betas.shape != (self.repetitions,):
            raise ValueError("'chain_betas' must hold {} inverse temperatures".format(self.repetitions))
        if not np.all(np.isfinite(chain_betas) & (chain_betas >= 0.0)):
            raise ValueError("'chain_betas' must be finite and not negative")
        return chain_betas

    def advance_ladder(self, chain_betas, number_sweeps: int, sweep_order: Optional[str] = None,
                       trace: bool = False):
        """Run ``number_sweeps`` more sweeps with chain ``r`` at inverse temperature ``chain_betas[r]``
        throughout (``asp_sa_chains_advance_ladder``, the ladder law of DESIGN.md §4.10): chain ``r``
        ends exactly where ``advance(np.full(number_sweeps, chain_betas[r]))`` would take it on a
        handle of its own.  ``sweep_order`` and ``trace`` as in ``advance``."""
        order = self._ORDERS[resolve_sweep_order(sweep_order)]
        chain_betas = self._chain_betas(chain_betas)
        number_sweeps = int(number_sweeps)
        if not 0 <= number_sweeps < 2**32:
            raise ValueError("'number_sweeps' must be a number of sweeps")
        handle = self._live()
        rows = np.zeros((self.repetitions, number_sweeps + 1), dtype=np.int64) if trace else None
        _lib.check(_lib.load().asp_sa_chains_advance_ladder(handle, _lib.ptr(chain_betas),
                                                            ctypes.c_uint32(number_sweeps), ctypes.c_uint32(order),
                                                            _lib.ptr(rows)))
        return rows

    def exchange(self, chain_betas, parity: int, draw: int = 0):
        """One replica-exchange step (law ASP-PT-1) on the device: the slots ``k`` and
        ``k + 1`` for every ``k`` of parity ``parity`` swap their configurations with probability
        ``min(1, exp((beta[k+1] - beta[k]) * (E[k+1] - E[k])))``; the temperatures stay with the slots.
        Returns ``(source uint32[R], energies float64[R], accepted)``: the slot every slot's state was
        taken from, the energies before the step and the number of pairs that swapped.  ``draw`` picks
        the random words (a Philox counter word), for more than one step at one sweep count."""
        chain_betas = self._chain_betas(chain_betas)
        parity, draw = int(parity), int(draw)
        if parity not in (0, 1):
            raise ValueError("'parity' must be 0 or 1")
        if not 0 <= draw < 2**32:
            raise ValueError("'draw' must fit 32 bits")
        handle = self._live()
        source = np.zeros(self.repetitions, dtype=np.uint32)
        energies = np.zeros(self.repetitions, dtype=np.float64)
        accepted = ctypes.c_uint32(0)
        _lib.check(_lib.load().asp_sa_chains_exchange(handle, _lib.ptr(chain_betas), ctypes.c_uint32(parity),
                                                      ctypes.c_uint32(draw), _lib.ptr(source), _lib.ptr(energies),
                                                      ctypes.byref(accepted)))
        return source, energies, int(accepted.value)

    def cluster_move(self, pairs, draw: int = 0):
        """One isoenergetic cluster move (Houdayer's move; law ASP-ICM-1) per pair on the
        device: the chains ``a`` and ``b`` of every row ``(a, b)`` of ``pairs`` — an ``(P, 2)`` array-like of
        slots, each named at most once; pair slots of equal temperature — flip one connected cluster of the
        sites on which their current configurations differ.  The sum of the two energies is conserved and
        nothing is rejected.  Returns ``(differing uint32[P], sizes uint32[P], deltas int64[P])``: the
        number of differing sites, the size of the flipped cluster and the change of chain ``a``'s tracked
        energy (chain ``b``'s is the opposite).  ``draw`` picks the random words (a Philox counter word),
        for more than one move at one sweep count; the same move again undoes it."""
        pairs = self._cluster_pairs(pairs)
        draw = int(draw)
        if not 0 <= draw < 2**32:
            raise ValueError("'draw' must fit 32 bits")
        handle = self._live()
        count = pairs.shape[0]
        differing = np.zeros(count, dtype=np.uint32)
        sizes = np.zeros(count, dtype=np.uint32)
        deltas = np.zeros(count, dtype=np.int64)
        _lib.check(_lib.load().asp_sa_chains_cluster_move(handle, _lib.ptr(pairs), ctypes.c_uint32(count),
                                                          ctypes.c_uint32(draw), _lib.ptr(differing),
                                                          _lib.ptr(sizes), _lib.ptr(deltas)))
        return differing, sizes, deltas

    def _cluster_pairs(self, pairs) -> np.ndarray:
        """``pairs`` of :meth:`cluster_move` checked, as a contiguous ``uint32[P, 2]``."""
        pairs = np.asarray(pairs)
        if pairs.size == 0:
            pairs = np.zeros((0, 2), dtype=np.uint32)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
            raise ValueError("'pairs' must be an (P, 2) array of chain indices")
        if np.any(pairs < 0) or np.any(pairs >= self.repetitions):
            raise ValueError("'pairs' must hold chain indices below {}".format(self.repetitions))
        if np.unique(pairs).size != pairs.size:
            raise ValueError("'pairs' names a chain more than once")
        return np.ascontiguousarray(pairs, dtype=np.uint32)

    def result(self, only_best: bool = False):
        """The best configuration so far of every chain and its energy, ``(xs[R, words], es[R])`` —
        what ``anneal(..., only_best=False)`` returns; ``only_best=True``: the best of them."""
        xs = np.zeros((self.repetitions, max(self.words, 1)), dtype=np.uint64)
        es = np.zeros(self.repetitions, dtype=np.float64)
        _lib.check(_lib.load().asp_sa_chains_result(self._live(), _lib.ptr(xs), _lib.ptr(es)))
        xs = xs[:, :self.words]
        if only_best:
            best = int(np.argmin(es))  # first minimum, as anneal()
            return xs[best].copy(), float(es[best])
        return xs, es

    _WHICH = {"best": 0, "current": 1}

    def scores(self, exact, weights=None, select=None, which: str = "best"):
        """``scores.sign_scores`` of the handle's configurations WHERE THEY ARE (``asp_sa_chains_scores``,
        specification ASP-SCORE-1): ``(matches uint64[R], signed float64[R], total)`` of
        every chain's best (``which="best"``) or current (``"current"``) configuration against ``exact``
        and ``weights``, position ``i`` taking spin ``select[i]`` (``None``: all spins in order).  Nothing
        is exported and the chains are not touched: what follows is bit for bit what follows without."""
        from . import scores as _scores

        if which not in self._WHICH:
            raise ValueError("'which' must be 'best' or 'current'")
        item = _scores._Item(None, exact, weights, select, self.hamiltonian.size, resident=True)
        item._outputs(self.repetitions)
        _lib.check(_lib.load().asp_sa_chains_scores(self._live(), ctypes.c_uint32(self._WHICH[which]),
                                                    ctypes.c_uint64(item.scored), _lib.ptr(item.select),
                                                    _lib.ptr(item.exact), _lib.ptr(item.weights),
                                                    _lib.ptr(item.matches), _lib.ptr(item.signed),
                                                    _lib.ptr(item.total)))
        return item.result()

    def accuracy_and_overlap(self, exact, weights=None, select=None, which: str = "best"):
        """``(accuracy float64[R], overlap float64[R])`` from :meth:`scores`."""
        from . import scores as _scores

        matches, signed, total = self.scores(exact, weights, select, which)
        scored = self.hamiltonian.size if select is None else np.asarray(select).reshape(-1).shape[0]
        return _scores.accuracy_and_overlap_of(matches, signed, total, scored)

    def distances(self, which: str = "best") -> np.ndarray:
        """``uint32[R, R]``: the Hamming distances between the chains' best (or current) configurations,
        computed where they are (``asp_sa_chains_distances``)."""
        if which not in self._WHICH:
            raise ValueError("'which' must be 'best' or 'current'")
        out = np.zeros((self.repetitions, self.repetitions), dtype=np.uint32)
        _lib.check(_lib.load().asp_sa_chains_distances(self._live(), ctypes.c_uint32(self._WHICH[which]),
                                                       _lib.ptr(out)))
        return out

    def consensus(self, weights=None, which: str = "best", anchor=None, align=None, rounds: int = 1):
        """``scores.consensus`` of the handle's configurations WHERE THEY ARE (``asp_sa_chains_vote_batch``,
        law ASP-VOTE-1): the chains' best (or current) configurations aligned up to the
        global flip and voted per site, as a ``scores.Consensus`` that also carries the ``energy`` of the
        consensus.  ``anchor=None``: the first chain of lowest energy, as ``result(only_best=True)`` picks
        it (that takes the energies through ``result()``; an explicit ``anchor`` exports nothing);
        ``align=None``: ``True`` exactly when the model has no field.  The chains are not touched."""
        return consensus_chains([self], weights=[weights], which=which, anchor=anchor, align=align, rounds=rounds)[0]

    def _export(self, names) -> dict:
        shapes ={"x_current": (self.repetitions, self.words), "x_best": (self.repetitions, self.words),
                  "tracked_current": (self.repetitions,), "tracked_best": (self.repetitions,),
                  "accepted": (self.repetitions,)}
        out = {name: np.zeros(shapes[name], dtype=np.int64 if name.startswith("tracked") else np.uint64)
               for name in names}
        snap = _lib.SaChainsSnapshot()
        for name, array in out.items():
            if array.size:
                setattr(snap, name, array.ctypes.data)
        _lib.check(_lib.load().asp_sa_chains_export(self._live(), ctypes.byref(snap)))
        out["sweeps_done"] = np.uint32(snap.sweeps_done)
        return out

    def state(self) -> dict:
        """Everything a continuation needs, as numpy arrays (``np.savez(path, **chains.state())``):
        ``x_current`` / ``x_best`` ``uint64[R, words]``, ``tracked_current`` / ``tracked_best``
        ``int64[R]`` (units of ``2**-energy_scale_exp``, relative to the chain's first
        configuration), ``accepted`` ``uint64[R]`` and ``sweeps_done``."""
        return self._export(["x_current", "x_best", "tracked_current", "tracked_best", "accepted"])

    def load_state(self, state) -> None:
        """Continue from ``state`` (a ``state()`` dict or the ``np.load`` of one) — chains of the same
        Hamiltonian, seed, repetitions and replica_offset."""
        shapes = {"x_current": (self.repetitions, self.words), "x_best": (self.repetitions, self.words),
                  "tracked_current": (self.repetitions,), "tracked_best": (self.repetitions,),
                  "accepted": (self.repetitions,)}
        snap = _lib.SaChainsSnapshot()
        keep = []
        for name, shape in shapes.items():
            dtype = np.int64 if name.startswith("tracked") else np.uint64
            array = np.ascontiguousarray(state[name], dtype=dtype)
            if array.shape != shape:
                raise ValueError("state[{!r}] must have shape {}".format(name, shape))
            if array.size == 0:
                array = np.zeros(1, dtype=dtype)  # (never read; a snapshot array must not be NULL)
            keep.append(array)
            setattr(snap, name, array.ctypes.data)
        sweeps_done = int(state["sweeps_done"])
        if not 0 <= sweeps_done < 2**32:
            raise ValueError("state['sweeps_done'] must fit 32 bits")
        snap.sweeps_done = sweeps_done
        _lib.check(_lib.load().asp_sa_chains_import(self._live(), ctypes.byref(snap)))

    def gather(self, source) -> None:
        """Slot ``j`` of all five state arrays becomes slot ``source[j]`` (``asp_sa_chains_gather``,
        DESIGN.md §4.11) — what ``load_state`` of the fancy-indexed ``state()`` does, on the device.
        Any map of ``repetitions`` entries below ``repetitions``: repeats, cycles, a reversal."""
        source = np.asarray(source)
        if source.shape != (self.repetitions,) or source.dtype.kind not in "iu":
            raise ValueError("'source' must hold {} chain indices".format(self.repetitions))
        if np.any(source < 0) or np.any(source >= 2**32):
            raise ValueError("'source' must hold chain indices")
        source = np.ascontiguousarray(source, dtype=np.uint32)
        _lib.check(_lib.load().asp_sa_chains_gather(self._live(), _lib.ptr(source)))

    def resample(self, dbeta: float, draw: int = 0):
        """One population-annealing step (law ASP-PA-1): the chains are weighted by
        ``exp(-dbeta * E)`` of their current configurations and resampled systematically on the
        device.  Returns ``(source uint32[R], energies float64[R], survivors)``: the chain every slot
        was taken from, the energies before the step and the number of distinct sources.  ``draw``
        picks the random offset (a Philox counter word), for more than one step at one sweep count."""
        return resample_chains([self], [dbeta], [draw])[0]

    def close(self) -> None:
        """Destroy the device handle now."""
        if self._handle is not None:
            try:
                _lib.load().asp_sa_chains_destroy(self._handle)
            finally:
                self._handle = None

    release = close  # (what _lib.shutdown calls on every live owner of a handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        if getattr(self, "_handle", None) is None or _lib.closed():
            return
        try:
            self.close()
        except Exception:
            pass


def anneal_until(hamiltonian: Hamiltonian, x0=None, seed=None, number_sweeps: int = 5120,
                 beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 1,
                 only_best: bool = True, sweep_order: Optional[str] = None, check_every: int = 512,
                 patience: Optional[int] = None, target=None):
    """``anneal`` that may stop early: the usual geometric ladder of ``number_sweeps`` sweeps is run
    in segments of ``check_every`` sweeps (``Chains``), and the run ends once NO chain's best energy
    has improved for ``patience`` consecutive segments.  Returns ``(x, e, sweeps_run)`` with
    ``(x, e)`` as ``anneal`` returns them.  ``patience=None`` never stops early and returns exactly
    ``anneal(...)``'s result (the continuation law).  Chains stay on this rank.

    ``target=(exact, weights, accuracy)``: the run also ends after the first segment at which some
    chain's best configuration has a sign accuracy (up to a global flip) of at least ``accuracy``
    against the packed signs ``exact`` — scored on the device, where the chains are (``Chains.scores``;
    ``weights`` may be ``None``).  ``target=None`` is the run without it."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError("'check_every' must be positive")
    if patience is not None and int(patience) < 1:
        raise ValueError("'patience' must be positive or None")
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    target = _check_target(target)
    if beta0 is None or beta1 is None:
        info = hamiltonian.info()
        beta0 = info.beta0_auto if beta0 is None else beta0
        beta1 = info.beta1_auto if beta1 is None else beta1
    betas = make_schedule(float(beta0), float(beta1), number_sweeps)
    with Chains(hamiltonian, seed=seed, repetitions=repetitions, x0=x0) as chains:
        best = chains._export(["tracked_best"])["tracked_best"]
        still = 0
        done = 0
        while done < betas.shape[0]:
            chains.advance(betas[done:done + check_every], sweep_order=order)
            done = min(done + check_every, betas.shape[0])
            now = chains._export(["tracked_best"])["tracked_best"]
            still = 0 if np.any(now < best) else still + 1
            best = now
            if patience is not None and still >= int(patience):
                break
            if target is not None and _target_met(chains, target):
                break
        x, e = chains.result(only_best=only_best)
    return x, e, done


def _check_target(target):
    if target is None:
        return None
    exact, weights, accuracy = target
    accuracy = float(accuracy)
    if not 0.0 <= accuracy <= 1.0:
        raise ValueError("a target's accuracy must lie in [0, 1]")
    return exact, weights, accuracy


def _target_met(chains: "Chains", target) -> bool:
    """Whether some chain's best configuration reaches the target's accuracy."""
    exact, weights, wanted = target
    accuracy, _ = chains.accuracy_and_overlap(exact, weights)
    return bool(np.any(accuracy >= wanted))


def advance_chains(chains, betas, sweep_order=None, progress: bool = False):
    """``chains[i].advance(betas[i], sweep_order[i])`` for every ``i`` in ONE device call
    (``asp_sa_chains_advance_batch``): exactly the same chains, but the handles share
    launches the way the problems of ``anneal_batch`` do.  ``chains``: ``Chains`` of distinct
    Hamiltonians; ``betas``: one array per handle (lengths may differ, an empty one runs nothing);
    ``sweep_order``: one value for all or one per handle.  ``progress=True`` returns
    ``[(tracked_best int64[R], improved), ...]``: every chain's best tracked energy after the segment
    and the number of chains whose best fell during it — one copy for the whole batch, no export per
    handle; else ``None``."""
    chains = list(chains)
    n = len(chains)
    for c in chains:
        if not isinstance(c, Chains):
            raise TypeError("'chains' must hold Chains objects")
    if isinstance(sweep_order, (list, tuple)):
        orders = list(sweep_order)
    else:
        orders = [sweep_order] * n
    betas = list(betas)
    if not (len(betas) == len(orders) == n):
        raise ValueError("advance_chains: %d handles, %d beta arrays and %d sweep orders" % (n, len(betas), len(orders)))
    betas = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1) for b in betas]
    orders = [Chains._ORDERS[resolve_sweep_order(o)] for o in orders]
    items = (_lib.SaChainsItem * max(n, 1))()
    out = []  # (also keeps the output buffers alive over the call)
    for i, c in enumerate(chains):
        items[i].chains = c._live()
        items[i].betas = betas[i].ctypes.data if betas[i].shape[0] else None
        items[i].num_sweeps = betas[i].shape[0]
        items[i].order = orders[i]
        items[i].flags = 0
        if progress:
            best = np.zeros(max(c.repetitions, 1), dtype=np.int64)
            improved = ctypes.c_uint32(0)
            items[i].out_tracked_best = best.ctypes.data
            items[i].out_improved = ctypes.addressof(improved)
            out.append((best, improved, c.repetitions))
    _lib.check(_lib.load().asp_sa_chains_advance_batch(items, ctypes.c_uint32(n)))
    if not progress:
        return None
    return [(best[:reps], int(improved.value)) for best, improved, reps in out]


def anneal_batch_until(hamiltonians, seed=None, number_sweeps: int = 5120, repetitions: int = 64,
                       only_best: bool = True, beta0: Optional[float] = None, beta1: Optional[float] = None,
                       sweep_order: Optional[str] = None, check_every: int = 512,
                       patience: Optional[int] = None, target=None):
    """``[anneal_until(h, seed=seed, number_sweeps=..., repetitions=..., ...) for h in hamiltonians]``
    with every segment of all problems still running in one device call (``advance_chains``): problem
    ``i`` stops once none of its chains improved for ``patience`` consecutive segments and is left out
    of the later calls.  Returns ``[(x, e, sweeps_run), ...]``; with ``patience=None`` nothing stops
    early and ``(x, e)`` is ``anneal_batch(...)``'s element.  ``seed`` as in ``anneal_batch``.
    ``target``: ``None``, or one ``(exact, weights, accuracy)`` (or ``None``) per problem as in
    ``anneal_until``: a problem also stops after the segment at which one of its chains meets it."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    check_every = int(check_every)
    if check_every < 1:
        raise ValueError("'check_every' must be positive")
    if patience is not None and int(patience) < 1:
        raise ValueError("'patience' must be positive or None")
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    for h in hamiltonians:
        if not isinstance(h, Hamiltonian):
            raise TypeError("'hamiltonians' must hold Hamiltonian objects")
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("anneal_batch_until: every problem needs its own Hamiltonian object")
    targets = [None] * n if target is None else [_check_target(t) for t in target]
    if len(targets) != n:
        raise ValueError("anneal_batch_until: %d problems and %d targets" % (n, len(targets)))
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    if seed is None or np.ndim(seed) == 0:
        seeds = [_resolve_seed(seed) for _ in range(n)] if seed is None else [_resolve_seed(seed)] * n
    else:
        seeds = [_resolve_seed(x) for x in seed]
    schedules = []
    for h in hamiltonians:
        b0, b1 = beta0, beta1
        if b0 is None or b1 is None:
            info = h.info()
            b0 = info.beta0_auto if b0 is None else b0
            b1 = info.beta1_auto if b1 is None else b1
        schedules.append(make_schedule(float(b0), float(b1), number_sweeps))
    handles = []
    try:
        for h, s in zip(hamiltonians, seeds):
            handles.append(Chains(h, seed=s, repetitions=repetitions))
        still = [0] * n
        done = [0] * n
        running = [i for i in range(n) if schedules[i].shape[0] > 0]
        while running:
            told = advance_chains([handles[i] for i in running],
                                  [schedules[i][done[i]:done[i] + check_every] for i in running],
                                  sweep_order=order, progress=True)
            later = []
            for i, (_, improved) in zip(running, told):
                done[i] = min(done[i] + check_every, schedules[i].shape[0])
                still[i] = 0 if improved else still[i] + 1
                if done[i] >= schedules[i].shape[0] or (patience is not None and still[i] >= int(patience)):
                    continue
                if targets[i] is not None and _target_met(handles[i], targets[i]):
                    continue
                later.append(i)
            running = later
        results = []
        for i, c in enumerate(handles):
            x, e = c.result(only_best=only_best)
            results.append((x, e, done[i]))
    finally:
        for c in handles:
            c.close()
    return results


def resample_chains(chains, dbetas, draws=0):
    """``chains[i].resample(dbetas[i], draws[i])`` for every ``i`` in ONE device call
    (``asp_sa_chains_resample_batch``): the same bits, but weights, selection and the
    gather of all handles share launches and every output comes back in one copy.  ``chains``:
    ``Chains`` of distinct Hamiltonians; ``dbetas`` and ``draws``: one value for all or one per handle.
    Returns ``[(source, energies, survivors), ...]``."""
    chains = list(chains)
    n = len(chains)
    for c in chains:
        if not isinstance(c, Chains):
            raise TypeError("'chains' must hold Chains objects")
    dbetas = [float(dbetas)] * n if np.ndim(dbetas) == 0 else [float(d) for d in dbetas]
    draws = [int(draws)] * n if np.ndim(draws) == 0 else [int(d) for d in draws]
    if not (len(dbetas) == len(draws) == n):
        raise ValueError("resample_chains: %d handles, %d steps and %d draws" % (n, len(dbetas), len(draws)))
    if any(not 0 <= d < 2**32 for d in draws):
        raise ValueError("'draws' must fit 32 bits")
    items = (_lib.SaChainsResampleItem * max(n, 1))()
    out = []  # (also keeps the output buffers alive over the call)
    for i, c in enumerate(chains):
        source = np.zeros(c.repetitions, dtype=np.uint32)
        energies = np.zeros(c.repetitions, dtype=np.float64)
        survivors = ctypes.c_uint32(0)
        items[i].chains = c._live()
        items[i].dbeta = dbetas[i]
        items[i].draw = draws[i]
        items[i].flags = 0
        items[i].out_source = source.ctypes.data
        items[i].out_energy = energies.ctypes.data
        items[i].out_survivors = ctypes.addressof(survivors)
        out.append((source, energies, survivors))
    _lib.check(_lib.load().asp_sa_chains_resample_batch(items, ctypes.c_uint32(n)))
    return [(source, energies, int(survivors.value)) for source, energies, survivors in out]


def population_anneal_batch(hamiltonians, seed=None, number_steps: int = 512, sweeps_per_step: int = 10,
                            beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 64,
                            only_best: bool = True, sweep_order: Optional[str] = None, resample: bool = True):
    """``[population_anneal(h, seed=seed, ...) for h in hamiltonians]`` with every step of all problems
    in one ``advance_chains`` call and one ``resample_chains`` call — identical results.  ``seed`` as
    in ``anneal_batch``.  Chains stay on this rank."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    number_steps, sweeps_per_step = int(number_steps), int(sweeps_per_step)
    if number_steps < 1 or sweeps_per_step < 1:
        raise ValueError("'number_steps' and 'sweeps_per_step' must be positive")
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    for h in hamiltonians:
        if not isinstance(h, Hamiltonian):
            raise TypeError("'hamiltonians' must hold Hamiltonian objects")
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("population_anneal_batch: every problem needs its own Hamiltonian object")
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    if seed is None or np.ndim(seed) == 0:
        seeds = [_resolve_seed(seed) for _ in range(n)] if seed is None else [_resolve_seed(seed)] * n
    else:
        seeds = [_resolve_seed(x) for x in seed]
    ladders = []
    for h in hamiltonians:
        b0, b1 = beta0, beta1
        if b0 is None or b1 is None:
            info = h.info()
            b0 = info.beta0_auto if b0 is None else b0
            b1 = info.beta1_auto if b1 is None else b1
        ladders.append(make_schedule(float(b0), float(b1), number_steps))
    handles = []
    try:
        for h, s in zip(hamiltonians, seeds):
            handles.append(Chains(h, seed=s, repetitions=repetitions))
        for k in range(number_steps):
            if resample and k >= 1:
                resample_chains(handles, [ladder[k] - ladder[k - 1] for ladder in ladders], 0)
            advance_chains(handles, [np.full(sweeps_per_step, ladder[k]) for ladder in ladders], sweep_order=order)
        results = [c.result(only_best=only_best) for c in handles]
    finally:
        for c in handles:
            c.close()
    return results


def population_anneal(hamiltonian: Hamiltonian, seed=None, number_steps: int = 512, sweeps_per_step: int = 10,
                      beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 64,
                      only_best: bool = True, sweep_order: Optional[str] = None, resample: bool = True):
    """Population annealing: ``repetitions`` chains visit the temperatures
    ``np.geomspace(beta0, beta1, number_steps)`` (the automatic defaults of ``anneal``) with
    ``sweeps_per_step`` sweeps at each, and before every step but the first they are reweighted by
    ``exp(-(beta_k - beta_{k-1}) E)`` and resampled on the device (``Chains.resample``, draw 0), so that
    low-energy chains are cloned into the slots of high-energy ones — the same sweeps as ``anneal``
    with ``number_steps * sweeps_per_step`` of them.  Returns what ``anneal`` returns.
    ``resample=False`` is exactly ``anneal`` on the schedule ``np.repeat(temperatures,
    sweeps_per_step)`` (the continuation law, §4.10).  Chains stay on this rank."""
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    return population_anneal_batch([hamiltonian], seed, number_steps, sweeps_per_step, beta0, beta1, repetitions,
                                   only_best, sweep_order, resample)[0]


def parallel_tempering(hamiltonian: Hamiltonian, seed=None, number_rounds: int = 512, sweeps_per_round: int = 10,
                       beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 64,
                       only_best: bool = True, sweep_order: Optional[str] = None, exchange: bool = True):
    """Parallel tempering: ``repetitions`` chains sit on the temperature ladder
    ``make_schedule(beta0, beta1, repetitions)`` (the automatic defaults of ``anneal``), slot ``k`` at
    ``ladder[k]`` throughout.  Round ``j`` is ``sweeps_per_round`` sweeps of every chain at its own
    temperature (``Chains.advance_ladder``) followed — except after the last round — by a
    replica-exchange step between neighbouring slots on the device (``Chains.exchange`` with parity
    ``j & 1``, draw 0).  Returns what ``anneal`` returns.  ``exchange=False`` is ``repetitions``
    independent constant-temperature chains (the ladder law, §4.10).  Chains stay on this rank."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    number_rounds, sweeps_per_round = int(number_rounds), int(sweeps_per_round)
    if number_rounds < 1 or sweeps_per_round < 1:
        raise ValueError("'number_rounds' and 'sweeps_per_round' must be positive")
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    if beta0 is None or beta1 is None:
        info = hamiltonian.info()
        beta0 = info.beta0_auto if beta0 is None else beta0
        beta1 = info.beta1_auto if beta1 is None else beta1
    ladder = make_schedule(float(beta0), float(beta1), repetitions)
    with Chains(hamiltonian, seed=seed, repetitions=repetitions) as chains:
        for j in range(number_rounds):
            chains.advance_ladder(ladder, sweeps_per_round, sweep_order=order)
            if exchange and j + 1 < number_rounds:
                chains.exchange(ladder, j & 1, 0)
        return chains.result(only_best=only_best)


def parallel_tempering_cluster(hamiltonian: Hamiltonian, seed=None, number_rounds: int = 512,
                               sweeps_per_round: int = 10, beta0: Optional[float] = None,
                               beta1: Optional[float] = None, repetitions: int = 64, only_best: bool = True,
                               sweep_order: Optional[str] = None, exchange: bool = True, cluster_rungs=None):
    """Parallel tempering with isoenergetic cluster moves: ``repetitions`` (even) chains,
    two per rung of the ladder ``make_schedule(beta0, beta1, repetitions // 2)`` laid out as a hairpin —
    slot ``k`` and slot ``repetitions - 1 - k`` both run at ``ladder[k]``.  Round ``j`` is
    ``Chains.advance_ladder``, then ``Chains.cluster_move`` of the pairs ``(k, repetitions - 1 - k)`` of
    the coldest ``cluster_rungs`` rungs (``None``: all of them) with draw 0 — on every round, the last
    included — and, except after the last round, ``Chains.exchange(hairpin, j & 1, 0)``.  Returns what
    ``anneal`` returns.  Chains stay on this rank."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    number_rounds, sweeps_per_round = int(number_rounds), int(sweeps_per_round)
    if number_rounds < 1 or sweeps_per_round < 1:
        raise ValueError("'number_rounds' and 'sweeps_per_round' must be positive")
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    repetitions = int(repetitions)
    if repetitions < 2 or repetitions % 2:
        raise ValueError("'repetitions' must be even and positive: two chains per rung")
    rungs = repetitions // 2
    cluster_rungs = rungs if cluster_rungs is None else int(cluster_rungs)
    if not 0 <= cluster_rungs <= rungs:
        raise ValueError("'cluster_rungs' must be between 0 and {}".format(rungs))
    if beta0 is None or beta1 is None:
        info = hamiltonian.info()
        beta0 = info.beta0_auto if beta0 is None else beta0
        beta1 = info.beta1_auto if beta1 is None else beta1
    ladder = make_schedule(float(beta0), float(beta1), rungs)
    hairpin = np.concatenate([ladder, ladder[::-1]])
    # (the ladder runs hot to cold: the coldest rungs are the last ones)
    pairs = np.array([(k, repetitions - 1 - k) for k in range(rungs - cluster_rungs, rungs)],
                     dtype=np.uint32).reshape(-1, 2)
    with Chains(hamiltonian, seed=seed, repetitions=repetitions) as chains:
        for j in range(number_rounds):
            chains.advance_ladder(hairpin, sweeps_per_round, sweep_order=order)
            chains.cluster_move(pairs, 0)
            if exchange and j + 1 < number_rounds:
                chains.exchange(hairpin, j & 1, 0)
        return chains.result(only_best=only_best)


def _per_handle(value, n: int, name: str) -> list:
    """``value`` as a list of ``n``: one value for all handles or one per handle."""
    if isinstance(value, (list, tuple, np.ndarray)):
        values = list(value)
        if len(values) != n:
            raise ValueError("%s: %d handles, %d values" % (name, n, len(values)))
        return values
    return [value] * n


def advance_ladder_chains(chains, chain_betas, number_sweeps, sweep_order=None, progress: bool = False):
    """``chains[i].advance_ladder(chain_betas[i], number_sweeps[i], sweep_order[i])`` for every ``i`` in
    ONE device call (``asp_sa_chains_advance_ladder_batch``): exactly the same chains,
    but the handles share launches the way ``advance_chains``' do.  ``chains``: ``Chains`` of distinct
    Hamiltonians; ``chain_betas``: one array of ``repetitions`` inverse temperatures per handle;
    ``number_sweeps`` and ``sweep_order``: one value for all or one per handle.  Returns what
    ``advance_chains`` returns."""
    chains = list(chains)
    n = len(chains)
    for c in chains:
        if not isinstance(c, Chains):
            raise TypeError("'chains' must hold Chains objects")
    chain_betas = list(chain_betas)
    if len(chain_betas) != n:
        raise ValueError("advance_ladder_chains: %d handles, %d ladders" % (n, len(chain_betas)))
    sweeps = [int(k) for k in _per_handle(number_sweeps, n, "advance_ladder_chains: 'number_sweeps'")]
    orders = _per_handle(sweep_order, n, "advance_ladder_chains: 'sweep_order'")
    if any(not 0 <= k < 2**32 for k in sweeps):
        raise ValueError("'number_sweeps' must be a number of sweeps")
    orders = [Chains._ORDERS[resolve_sweep_order(o)] for o in orders]
    ladders = [c._chain_betas(b) for c, b in zip(chains, chain_betas)]
    items = (_lib.SaChainsLadderItem * max(n, 1))()
    out = []  # (also keeps the output buffers alive over the call)
    for i, c in enumerate(chains):
        items[i].chains = c._live()
        items[i].chain_betas = ladders[i].ctypes.data
        items[i].num_sweeps = sweeps[i]
        items[i].order = orders[i]
        items[i].flags = 0
        if progress:
            best = np.zeros(max(c.repetitions, 1), dtype=np.int64)
            improved = ctypes.c_uint32(0)
            items[i].out_tracked_best = best.ctypes.data
            items[i].out_improved = ctypes.addressof(improved)
            out.append((best, improved, c.repetitions))
    _lib.check(_lib.load().asp_sa_chains_advance_ladder_batch(items, ctypes.c_uint32(n)))
    if not progress:
        return None
    return [(best[:reps], int(improved.value)) for best, improved, reps in out]


def exchange_chains(chains, chain_betas, parity, draws=0):
    """``chains[i].exchange(chain_betas[i], parity[i], draws[i])`` for every ``i`` in ONE device call
    (``asp_sa_chains_exchange_batch``): the same bits, but the selection and the gather
    of all handles share launches and every output comes back in one copy.  ``parity`` and ``draws``:
    one value for all or one per handle.  Returns ``[(source, energies, accepted), ...]``."""
    chains = list(chains)
    n = len(chains)
    for c in chains:
        if not isinstance(c, Chains):
            raise TypeError("'chains' must hold Chains objects")
    chain_betas = list(chain_betas)
    if len(chain_betas) != n:
        raise ValueError("exchange_chains: %d handles, %d ladders" % (n, len(chain_betas)))
    parities = [int(x) for x in _per_handle(parity, n, "exchange_chains: 'parity'")]
    draws = [int(x) for x in _per_handle(draws, n, "exchange_chains: 'draws'")]
    if any(x not in (0, 1) for x in parities):
        raise ValueError("'parity' must be 0 or 1")
    if any(not 0 <= d < 2**32 for d in draws):
        raise ValueError("'draws' must fit 32 bits")
    ladders = [c._chain_betas(b) for c, b in zip(chains, chain_betas)]
    items = (_lib.SaChainsExchangeItem * max(n, 1))()
    out = []  # (also keeps the output buffers alive over the call)
    for i, c in enumerate(chains):
        source = np.zeros(c.repetitions, dtype=np.uint32)
        energies = np.zeros(c.repetitions, dtype=np.float64)
        accepted = ctypes.c_uint32(0)
        items[i].chains = c._live()
        items[i].chain_betas = ladders[i].ctypes.data
        items[i].parity = parities[i]
        items[i].draw = draws[i]
        items[i].flags = 0
        items[i].out_source = source.ctypes.data
        items[i].out_energy = energies.ctypes.data
        items[i].out_accepted = ctypes.addressof(accepted)
        out.append((source, energies, accepted))
    _lib.check(_lib.load().asp_sa_chains_exchange_batch(items, ctypes.c_uint32(n)))
    return [(source, energies, int(accepted.value)) for source, energies, accepted in out]


CLUSTER_NO_PACKED = 1  # ASP_CLUSTER_NO_PACKED (include/asp.h): the workgroup-per-pair form for the handle


def cluster_move_chains(chains, pairs, draws=0, flags=0):
    """``chains[i].cluster_move(pairs[i], draws[i])`` for every ``i`` in ONE device call
    (``asp_sa_chains_cluster_move_batch``): the same bits, but the pairs of all handles
    share at most three launches — the pairs of small models (up to 2048 spins) a wavefront each — and every
    output comes back in one copy.  ``pairs``: one ``(P_i, 2)`` array-like per handle; ``draws``: one value
    for all or one per handle; ``flags`` (tests and timing; results do not depend on it): likewise,
    ``CLUSTER_NO_PACKED`` forces the workgroup form.  Returns ``[(differing, sizes, deltas), ...]``."""
    chains = list(chains)
    n = len(chains)
    for c in chains:
        if not isinstance(c, Chains):
            raise TypeError("'chains' must hold Chains objects")
    pairs = list(pairs)
    if len(pairs) != n:
        raise ValueError("cluster_move_chains: %d handles, %d arrays of pairs" % (n, len(pairs)))
    draws = [int(x) for x in _per_handle(draws, n, "cluster_move_chains: 'draws'")]
    flags = [int(x) for x in _per_handle(flags, n, "cluster_move_chains: 'flags'")]
    if any(not 0 <= d < 2**32 for d in draws):
        raise ValueError("'draws' must fit 32 bits")
    if any(f not in (0, CLUSTER_NO_PACKED) for f in flags):
        raise ValueError("'flags' must be 0 or CLUSTER_NO_PACKED")
    checked, known = [], {}  # (a driver hands every handle the same array: checked once per chain count)
    for c, p in zip(chains, pairs):
        key = (id(p), c.repetitions)
        if key not in known:
            known[key] = c._cluster_pairs(p)
        checked.append(known[key])
    items = (_lib.SaChainsClusterItem * max(n, 1))()
    out = []  # (also keeps the output buffers alive over the call)
    for i, c in enumerate(chains):
        count = checked[i].shape[0]
        differing = np.zeros(count, dtype=np.uint32)
        sizes = np.zeros(count, dtype=np.uint32)
        deltas = np.zeros(count, dtype=np.int64)
        items[i].chains = c._live()
        items[i].pairs = checked[i].ctypes.data
        items[i].num_pairs = count
        items[i].draw = draws[i]
        items[i].flags = flags[i]
        items[i].out_differing = differing.ctypes.data
        items[i].out_size = sizes.ctypes.data
        items[i].out_delta = deltas.ctypes.data
        out.append((differing, sizes, deltas))
    _lib.check(_lib.load().asp_sa_chains_cluster_move_batch(items, ctypes.c_uint32(n)))
    return out


def consensus_chains(chains, weights=None, which="best", anchor=None, align=None, rounds=1) -> list:
    """``chains[i].consensus(weights[i], which[i], anchor[i], align[i], rounds[i])`` for every ``i`` in ONE
    device call (``asp_sa_chains_vote_batch``): the same bits, but the handles share two
    launches a round and every output comes back in one copy.  ``weights``: ``None`` (all 1 everywhere)
    or one entry per handle (an array or ``None``); the others: one value for all or one per handle.  The
    call only reads, so a handle may be named more than once."""
    from . import scores as _scores

    chains = list(chains)
    n = len(chains)
    for c in chains:
        if not isinstance(c, Chains):
            raise TypeError("'chains' must hold Chains objects")
    weights = [None] * n if weights is None else list(weights)
    if len(weights) != n:
        raise ValueError("consensus_chains: %d handles, %d arrays of weights" % (n, len(weights)))
    whiches = _per_handle(which, n, "consensus_chains: 'which'")
    if any(w not in Chains._WHICH for w in whiches):
        raise ValueError("'which' must be 'best' or 'current'")
    anchors = _per_handle(anchor, n, "consensus_chains: 'anchor'")
    aligns = _per_handle(align, n, "consensus_chains: 'align'")
    all_rounds = _per_handle(rounds, n, "consensus_chains: 'rounds'")
    items = (_lib.SaChainsVoteItem * max(n, 1))()
    votes = []
    for i, c in enumerate(chains):
        handle = c._live()
        if anchors[i] is None:
            anchors[i] = int(np.argmin(c.result()[1]))  # first minimum, as result(only_best=True)
        if aligns[i] is None:
            aligns[i] = not np.any(c.hamiltonian.field)
        vote = _scores._Vote(c.hamiltonian.size, c.repetitions, weights[i], None, anchors[i], aligns[i], all_rounds[i])
        vote.fill(items[i])
        items[i].chains = handle
        items[i].which = Chains._WHICH[whiches[i]]
        votes.append(vote)
    _lib.check(_lib.load().asp_sa_chains_vote_batch(items, ctypes.c_uint32(n)))
    out = []
    for c, vote in zip(chains, votes):
        result = vote.result()
        result.energy = float(c.hamiltonian.energy(result.x))
        out.append(result)
    return out


def parallel_tempering_cluster_batch(hamiltonians, seed=None, number_rounds: int = 512, sweeps_per_round: int = 10,
                                     beta0: Optional[float] = None, beta1: Optional[float] = None,
                                     repetitions: int = 64, only_best: bool = True,
                                     sweep_order: Optional[str] = None, exchange: bool = True, cluster_rungs=None):
    """``[parallel_tempering_cluster(h, seed=seed, ...) for h in hamiltonians]`` with every round of all
    problems in one ``advance_ladder_chains`` call, one ``cluster_move_chains`` call (on every round, the
    last included) and — except after the last round — one ``exchange_chains`` call: identical results.
    ``seed`` as in ``anneal_batch``.  Chains stay on this rank."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    number_rounds, sweeps_per_round = int(number_rounds), int(sweeps_per_round)
    if number_rounds < 1 or sweeps_per_round < 1:
        raise ValueError("'number_rounds' and 'sweeps_per_round' must be positive")
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    for h in hamiltonians:
        if not isinstance(h, Hamiltonian):
            raise TypeError("'hamiltonians' must hold Hamiltonian objects")
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("parallel_tempering_cluster_batch: every problem needs its own Hamiltonian object")
    repetitions = int(repetitions)
    if repetitions < 2 or repetitions % 2:
        raise ValueError("'repetitions' must be even and positive: two chains per rung")
    rungs = repetitions // 2
    cluster_rungs = rungs if cluster_rungs is None else int(cluster_rungs)
    if not 0 <= cluster_rungs <= rungs:
        raise ValueError("'cluster_rungs' must be between 0 and {}".format(rungs))
    if seed is None or np.ndim(seed) == 0:
        seeds = [_resolve_seed(seed) for _ in range(n)] if seed is None else [_resolve_seed(seed)] * n
    else:
        seeds = [_resolve_seed(x) for x in seed]
    hairpins = []
    for h in hamiltonians:
        b0, b1 = beta0, beta1
        if b0 is None or b1 is None:
            info = h.info()
            b0 = info.beta0_auto if b0 is None else b0
            b1 = info.beta1_auto if b1 is None else b1
        ladder = make_schedule(float(b0), float(b1), rungs)
        hairpins.append(np.concatenate([ladder, ladder[::-1]]))
    # (the ladder runs hot to cold: the coldest rungs are the last ones)
    pairs = np.array([(k, repetitions - 1 - k) for k in range(rungs - cluster_rungs, rungs)],
                     dtype=np.uint32).reshape(-1, 2)
    handles = []
    try:
        for h, s in zip(hamiltonians, seeds):
            handles.append(Chains(h, seed=s, repetitions=repetitions))
        for j in range(number_rounds):
            advance_ladder_chains(handles, hairpins, sweeps_per_round, sweep_order=order)
            cluster_move_chains(handles, [pairs] * n, 0)
            if exchange and j + 1 < number_rounds:
                exchange_chains(handles, hairpins, j & 1, 0)
        results = [c.result(only_best=only_best) for c in handles]
    finally:
        for c in handles:
            c.close()
    return results


def parallel_tempering_batch(hamiltonians, seed=None, number_rounds: int = 512, sweeps_per_round: int = 10,
                             beta0: Optional[float] = None, beta1: Optional[float] = None, repetitions: int = 64,
                             only_best: bool = True, sweep_order: Optional[str] = None, exchange: bool = True):
    """``[parallel_tempering(h, seed=seed, ...) for h in hamiltonians]`` with every round of all problems
    in one ``advance_ladder_chains`` call and — except after the last round — one ``exchange_chains``
    call: identical results.  ``seed`` as in ``anneal_batch``.  Chains stay on this rank."""
    order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    number_rounds, sweeps_per_round = int(number_rounds), int(sweeps_per_round)
    if number_rounds < 1 or sweeps_per_round < 1:
        raise ValueError("'number_rounds' and 'sweeps_per_round' must be positive")
    hamiltonians = list(hamiltonians)
    n = len(hamiltonians)
    for h in hamiltonians:
        if not isinstance(h, Hamiltonian):
            raise TypeError("'hamiltonians' must hold Hamiltonian objects")
    if len({id(h) for h in hamiltonians}) != n:
        raise ValueError("parallel_tempering_batch: every problem needs its own Hamiltonian object")
    repetitions = int(repetitions)
    if repetitions < 1:
        raise ValueError("'repetitions' must be positive")
    if seed is None or np.ndim(seed) == 0:
        seeds = [_resolve_seed(seed) for _ in range(n)] if seed is None else [_resolve_seed(seed)] * n
    else:
        seeds = [_resolve_seed(x) for x in seed]
    ladders = []
    for h in hamiltonians:
        b0, b1 = beta0, beta1
        if b0 is None or b1 is None:
            info = h.info()
            b0 = info.beta0_auto if b0 is None else b0
            b1 = info.beta1_auto if b1 is None else b1
        ladders.append(make_schedule(float(b0), float(b1), repetitions))
    handles = []
    try:
        for h, s in zip(hamiltonians, seeds):
            handles.append(Chains(h, seed=s, repetitions=repetitions))
        for j in range(number_rounds):
            advance_ladder_chains(handles, ladders, sweeps_per_round, sweep_order=order)
            if exchange and j + 1 < number_rounds:
                exchange_chains(handles, ladders, j & 1, 0)
        results = [c.result(only_best=only_best) for c in handles]
    finally:
        for c in handles:
            c.close()
    return results


def anneal_with_traces(hamiltonian: Hamiltonian, x0=None, seed=None, number_sweeps: int = 5120,
                       beta0: Optional[float] = None, beta1: Optional[float] = None,
                       sweep_order: Optional[str] = "colour"):
    """The older annealer API (annealing_sign_problem/train.py:238-245, square_deep.py:181-183):
    one chain, ``(x, e_current, e_best)`` with the energy after every sweep and the best energy
    so far (``e_best[0]`` before the first sweep, ``e_best[-1]`` the returned configuration's).

    The traces come from the kernel's exact integer bookkeeping of the accepted ``dE`` and are
    anchored at the returned configuration's energy, which is recomputed in full precision.

    ``sweep_order="colour"`` (the default, what this function has always run) traces the fixed
    colour order — NOT the chain ``anneal(h, seed=seed)`` runs.  ``sweep_order=None`` gives the
    chain ``anneal()`` runs: ``$ASP_SWEEP_ORDER`` if set, else ``"shuffled"``, the reference
    annealer's order.  ``sweep_order="shuffled"`` asks for that order by name."""
    sweep_order = resolve_sweep_order(sweep_order)  # (first: a bad order fails without a GPU)
    if not isinstance(hamiltonian, Hamiltonian):
        raise TypeError("'hamiltonian' must be a Hamiltonian")
    xs, _, e_current, e_best = anneal_traces(hamiltonian, x0, seed, number_sweeps, beta0, beta1, 1,
                                             sweep_order)
    return xs[0].copy(), e_current[0], e_best[0]


def greedy_solve(hamiltonian: Hamiltonian, tree=None):
    """Strongest-coupling-first greedy sign assignment (common.py:250).  ``tree``: ``"host"`` or
    ``"device"``, where the strongest-coupling tree is built (``None``: ``$ASP_GREEDY_TREE`` or
    ``"host"``); the result does not depend on it."""
    from . import greedy as _greedy

    return _greedy.greedy_solve(hamiltonian, _greedy.MAX_RELAXATION_SWEEPS, tree)


def greedy_solve_batch(hamiltonians, max_sweeps=None, return_sweeps: bool = False, tree=None):
    """``[greedy_solve(h) for h in hamiltonians]`` in one device call (``asp_sa_greedy_batch``):
    identical results, the descents of all problems in shared launches.  ``tree``: as in
    :func:`greedy_solve` (with ``"device"`` the trees share launches too and never leave the device)."""
    from . import greedy as _greedy

    hamiltonians = list(hamiltonians)
    for h in hamiltonians:
        if not isinstance(h, Hamiltonian):
            raise TypeError("'hamiltonians' must hold Hamiltonian objects")
    return _greedy.greedy_solve_batch(
        hamiltonians, _greedy.MAX_RELAXATION_SWEEPS if max_sweeps is None else max_sweeps, return_sweeps, tree)
