"""Entry points of ``annealing_sign_problem.common`` on the MI355X path.

Same names, arguments and return values as the reference functions cited in
each docstring, so a caller of the reference (``process_cluster`` in
experiments/sampled_connected_components.py:726-751, the CLIs at
annealing_sign_problem/common.py:838-1002) can switch the import.  The two
numba kernels of the coupling build and the annealer run on the GPU through
libasp_hip.so; orchestration stays numpy/scipy exactly where the reference's is.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass
from typing import Any, Callable, Optional, Tuple

import numpy as np
import scipy.sparse

from . import _lib
from . import annealer as sa

__all__ = [
    "IsingModel",
    "make_ising_model",
    "make_ising_models",
    "reweight_ising_model",
    "reweight_ising_models",
    "solve_ising_model",
    "solve_ising_models",
    "dump_ising_model_to_hdf5",
    "load_ising_model_from_hdf5",
    "load_ground_state",
    "save_ground_state",
    "compute_accuracy_and_overlap",
    "compute_accuracies_and_overlaps",
    "make_hamiltonian_extension",
    "make_hamiltonian_extensions",
    "extension_spins",
    "extension_spins_segments",
    "extend_and_sparsify_models",
    "sparsify_component_segments",
    "sparsify_models_using_global_cutoff",
    "local_energies",
    "variational_energy",
    "sparsify_using_global_cutoff",
    "get_strongest_off_diag",
    "cluster_statistics",
    "coupling_distribution",
    "probability_of_frustration",
    "binary_search",
    "monte_carlo_sampling",
    "add_noise_to_amplitudes",
    "ground_state_to_log_coeff_fn",
    "norm2",
    "SamplingResult",
]

APPLY_CHUNK = 10000  # rows per batched_apply call (common.py:85)


@dataclass
class IsingModel:
    """common.py:46-55."""

    spins: np.ndarray
    quantum_hamiltonian: Any
    ising_hamiltonian: sa.Hamiltonian
    initial_signs: np.ndarray
    # (not in the reference) positions of `spins` in the basis, when the amplitude closure that
    # built the model looked them up: later stages of the pipeline reuse them instead of asking
    # the basis again
    basis_index: Optional[np.ndarray] = None

    @property
    def size(self) -> int:
        return self.spins.shape[0]


BLAS_THREADING_THRESHOLD = 10000  # OpenBLAS splits dot products longer than this over its threads


def dot(a: np.ndarray, b: np.ndarray) -> float:
    """``np.dot`` of two real vectors, kept off the BLAS thread pool.  Up to 10 000 elements it
    IS ``np.dot`` (one BLAS kernel on the calling thread: the reference's arithmetic).  Longer
    vectors OpenBLAS hands to its thread pool: the summation order then depends on the number of
    its threads, the call takes the library's global lock, so that the pipeline's --jobs threads
    queue up behind it, and the pool's workers keep spinning on the cores afterwards — measured
    on the sampled-cluster pipeline: 5 to 30 ms per call and every OTHER stage 2.5x slower
    (profiles/r03_pipeline_stages.txt).  Those go through numpy's pairwise summation: the same
    value to the last bit or two, on every machine, in 0.03 ms."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.shape[0] <= BLAS_THREADING_THRESHOLD:
        return float(np.dot(a, b))
    return float(np.add.reduce(a * b))


def norm2(x: np.ndarray) -> float:
    """Euclidean norm of a real vector: ``np.linalg.norm`` (= sqrt(dot(x, x)), common.py:166)
    through :func:`dot`."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] <= BLAS_THREADING_THRESHOLD:
        return float(np.linalg.norm(x))
    return float(np.sqrt(np.add.reduce(x * x)))


def _normalize_spins(spins) -> np.ndarray:
    """1-D keys -> C-contiguous (n, 8) zero-padded uint64 (common.py:58-68)."""
    from ._build_matrix import as_bits512

    return as_bits512(spins)


def _on_device(hamiltonian) -> bool:
    """True for this package's symmetry-free operators with real matrices (the stand-in for
    ``ls.Operator``): their action has a HIP implementation.  Foreign operator objects keep
    the reference's route through their own ``batched_apply``."""
    from . import operators

    return isinstance(hamiltonian, operators.Operator) and hamiltonian.is_real


def _batched_apply(hamiltonian, spins, chunk_size: int = APPLY_CHUNK):
    """Chunked ``hamiltonian.batched_apply`` returning flat
    ``(other_spins u64[N], other_coeffs f64[N], other_counts i64[K])`` (common.py:85-106)."""
    if hamiltonian.basis.number_spins > 64:
        raise AssertionError("TODO: only works with up to 64 bits")
    if _on_device(hamiltonian):
        # this package's own operator: the action runs on the GPU in one call
        flat = np.ascontiguousarray(np.asarray(spins, dtype=np.uint64).reshape(len(spins), -1)[:, 0])
        return hamiltonian.device().apply(flat)
    keys, coeffs, counts = [], [], []
    total = spins.shape[0]
    for start in range(0, total, chunk_size):
        block = _normalize_spins(spins[start:start + chunk_size])
        other, c, n = hamiltonian.batched_apply(block)
        c = np.asarray(c)
        if not np.allclose(c.imag, 0, atol=1e-6):
            raise ValueError("expected all Hamiltonian matrix elements to be real")
        keys.append(np.ascontiguousarray(np.asarray(other)[:, 0], dtype=np.uint64))
        coeffs.append(np.ascontiguousarray(c.real, dtype=np.float64))
        counts.append(np.asarray(n, dtype=np.int64))
    if not keys:
        return (np.zeros(0, np.uint64), np.zeros(0, np.float64), np.zeros(0, np.int64))
    return np.hstack(keys), np.hstack(coeffs), np.hstack(counts)


def ising_elements(keys, psi, other_keys, other_coeffs, other_counts):
    """GPU pass over the connections: ``(other_indices i64[N], member bool[N],
    elements f64[N], offsets i64[K+1])`` — the fused equivalent of
    ``_clipped_search_sorted`` (common.py:116-128), the membership test (:173)
    and ``_make_ising_model_compute_elements`` (:71-82)."""
    lib = _lib.load()
    _lib.require_gpu()
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    psi = np.ascontiguousarray(psi, dtype=np.float64)
    other_keys = np.ascontiguousarray(other_keys, dtype=np.uint64)
    other_coeffs = np.ascontiguousarray(other_coeffs, dtype=np.float64)
    other_counts = np.ascontiguousarray(other_counts, dtype=np.int64)
    k, n = keys.shape[0], other_keys.shape[0]
    indices = np.zeros(max(n, 1), dtype=np.int64)
    member = np.zeros(max(n, 1), dtype=np.uint8)
    elements = np.zeros(max(n, 1), dtype=np.float64)
    offsets = np.zeros(k + 1, dtype=np.int64)
    _lib.check(lib.asp_ising_elements(
        ctypes.c_uint64(k), _lib.ptr(keys), _lib.ptr(psi), ctypes.c_uint64(n), _lib.ptr(other_keys),
        _lib.ptr(other_coeffs), _lib.ptr(other_counts), _lib.ptr(indices), _lib.ptr(member),
        _lib.ptr(elements), _lib.ptr(offsets)))
    return indices[:n], member[:n].astype(bool), elements[:n], offsets


def _takes_host_route(error) -> bool:
    """A refusal of the fused coupling build after which the host route (``ising_elements`` + scipy)
    does the job: ASP_ERR_INVALID (duplicates with one-directional matrix elements), and the ONE
    ASP_ERR_TOO_LARGE of the emit pass whose rows do not fit the LDS of a workgroup — 1137 bonds or
    more, i.e. all-to-all models from 49 sites.  Any other size refusal stays an
    error."""
    return error.code == -3 or (error.code == -4 and "bytes of LDS" in str(error))


def make_ising_model(
    spins,
    quantum_hamiltonian,
    log_psi: Optional[np.ndarray] = None,
    log_psi_fn: Optional[Callable[[np.ndarray], np.ndarray]] = None,
    external_field: bool = False,
    debug: bool = False,
) -> IsingModel:
    """Auxiliary Ising model of a set of basis states (common.py:131-208).

    ``J = (M + M^T) / 2`` with ``M_ij = H_ij |psi_i| |psi_j|`` over the states of
    the cluster (psi L2-normalised over the cluster), zero field, and the signs of
    psi as the initial configuration.  ``external_field=True`` (`assert False` in the reference;
    this package's device operators only): the field is the boundary field of the cluster in its
    one-hop extension, ``h_r = 2 * sum_e H_er |psi_r| psi_e / c`` over the connections e that leave
    the cluster, amplitudes from ``log_psi_fn`` and c the cluster's norm, so that
    energy differences of the model are those of the full vector with the environment's signs
    kept.  One deliberate difference: for NON-unique
    input the reference indexes the already-deduplicated array with first-occurrence
    positions of the original (common.py:149), which is an indexing slip; here the
    sorted unique states are kept and ``log_psi`` is taken at first occurrences.
    """
    if log_psi is None and log_psi_fn is None:
        raise ValueError("at least one of log_psi or log_psi_fn should be specified")
    if external_field and log_psi_fn is None:
        raise ValueError("log_psi_fn should be specified when external_field=True")
    if external_field and not _on_device(quantum_hamiltonian):
        # the reference's branch is `assert False` (common.py:199-202); the field is built by the
        # device operator alone (DeviceOperator.field)
        raise NotImplementedError(
            "external_field=True needs one of this package's device operators (operators.Operator with "
            "real matrices); it is not implemented for foreign operator objects, nor by the reference")

    spins, log_psi, basis_index = _cluster_states(spins, log_psi, log_psi_fn)
    n = spins.shape[0]

    psi, field = _cluster_amplitudes_and_field(quantum_hamiltonian, spins, log_psi, log_psi_fn, external_field)
    matrix = None
    ising_hamiltonian = None
    if _on_device(quantum_hamiltonian):
        # action, search, elements and (M + M^T)/2 on the GPU, nothing materialised on the host
        # (csrc/operator_apply.hip): the pair-fused pass for operators whose rows reach distinct
        # states, the duplicate-keeping passes for symmetry-adapted bases.  Rows with duplicates
        # AND one-directional matrix elements are refused: host route below.
        try:
            # row-major, columns ascending, no duplicates (csrc/operator_apply.hip): canonical CSR
            indptr, col, val = quantum_hamiltonian.device().ising_csr(spins, psi)
            ising_hamiltonian = sa.Hamiltonian.from_canonical_csr(indptr, col, val, field)
        except _lib.AspError as error:
            if not _takes_host_route(error):
                raise
    if ising_hamiltonian is None:
        other_spins, other_coeffs, other_counts = _batched_apply(quantum_hamiltonian, spins)
        other_indices, _member, elements, offsets = ising_elements(
            spins, psi, other_spins, other_coeffs, other_counts)
        matrix = scipy.sparse.csr_matrix((elements, other_indices, offsets), shape=(n, n))
        matrix = 0.5 * (matrix + matrix.T)
        matrix.sort_indices()
        matrix = matrix.tocoo()
        ising_hamiltonian = sa.Hamiltonian(matrix, field)
    x0 = sa.signs_to_bits(np.sign(psi))
    return IsingModel(spins, quantum_hamiltonian, ising_hamiltonian, x0, basis_index)


def make_ising_models(clusters, quantum_hamiltonian, log_psis=None, log_psi_fn=None, external_field: bool = False):
    """``[make_ising_model(c, quantum_hamiltonian, log_psi=l, log_psi_fn=log_psi_fn,
    external_field=external_field) for c, l in zip(clusters, log_psis)]`` (not in the reference) with
    the couplings of ALL clusters built in one device call (``DeviceOperator.ising_csr_segments``,
    ASP-ISING-SEG-1): the same models field by field — ``spins``, the exchange's CSR
    arrays as bits, ``field``, ``initial_signs``, ``basis_index``.  Everything else is done per cluster
    as there: sort and unique, the amplitudes and their normalisation, the ``index_of`` / ``at_index``
    shortcut of the ground-state closure.  With ``external_field=True`` the boundary fields of ALL
    clusters come from one extension call and one field call (``_boundary_fields``, ASP-FIELD-SEG-1,
    DESIGN.md §3.5.1): ``log_psi_fn`` is asked for the environments cluster by cluster, in order, AFTER
    the states of all clusters instead of in turns with them, so a pure ``log_psi_fn`` gives identical
    models.  ``log_psis``: one array per cluster, or ``None``.  Foreign operator objects, and operators whose
    segmented call is refused with ASP_ERR_INVALID (one-directional matrix elements with duplicates),
    take the loop."""
    clusters = list(clusters)
    log_psis = [None] * len(clusters) if log_psis is None else list(log_psis)
    if len(log_psis) != len(clusters):
        raise ValueError("'log_psis' should hold one array per cluster")

    def loop():
        return [make_ising_model(c, quantum_hamiltonian, log_psi=l, log_psi_fn=log_psi_fn,
                                 external_field=external_field) for c, l in zip(clusters, log_psis)]

    if not _on_device(quantum_hamiltonian) or not clusters:
        return loop()
    if log_psi_fn is None and any(l is None for l in log_psis):
        raise ValueError("at least one of log_psi or log_psi_fn should be specified")
    if external_field and log_psi_fn is None:
        raise ValueError("log_psi_fn should be specified when external_field=True")
    states = []
    for spins, log_psi in zip(clusters, log_psis):
        spins, log_psi, basis_index = _cluster_states(spins, log_psi, log_psi_fn)
        psi, cluster_norm = _cluster_amplitudes(log_psi)
        states.append((spins, basis_index, psi, cluster_norm))
    if external_field:
        fields = _boundary_fields(quantum_hamiltonian, [(spins, psi, c) for spins, _, psi, c in states], log_psi_fn)
    else:
        fields = [np.zeros(spins.shape[0]) for spins, _, _, _ in states]
    prepared = [(spins, basis_index, psi, field) for (spins, basis_index, psi, _), field in zip(states, fields)]
    offsets = np.zeros(len(prepared) + 1, dtype=np.uint64)
    np.cumsum([p[0].shape[0] for p in prepared], out=offsets[1:])
    try:
        indptr, col, val = quantum_hamiltonian.device().ising_csr_segments(
            np.concatenate([p[0] for p in prepared]), np.concatenate([p[2] for p in prepared]), offsets)
    except _lib.AspError as error:
        if not _takes_host_route(error):
            raise
        return loop()
    models = []
    for g, (spins, basis_index, psi, field) in enumerate(prepared):
        first, last = int(offsets[g]), int(offsets[g + 1])
        begin, end = int(indptr[first]), int(indptr[last])
        # the global indptr rebased to the segment; the columns are local already
        hamiltonian = sa.Hamiltonian.from_canonical_csr(indptr[first:last + 1] - begin, col[begin:end].copy(),
                                                        val[begin:end].copy(), field)
        models.append(IsingModel(spins, quantum_hamiltonian, hamiltonian, sa.signs_to_bits(np.sign(psi)),
                                 basis_index))
    return models


def make_hamiltonian_extensions(models, log_psi_fn, external_field: bool = False):
    """``[make_hamiltonian_extension(m, log_psi_fn, external_field) for m in models]`` (not in the
    reference) with the couplings of all extensions — and, with ``external_field``, their boundary
    fields — built in one device call each (:func:`make_ising_models`); the models share one operator."""
    models = list(models)
    if not models:
        return []
    operator = models[0].quantum_hamiltonian
    if any(m.quantum_hamiltonian is not operator for m in models):
        return [make_hamiltonian_extension(m, log_psi_fn, external_field) for m in models]
    extended = [extension_spins(operator, m.spins) for m in models]
    return make_ising_models(extended, operator, log_psi_fn=log_psi_fn, external_field=external_field)


def _cluster_states(spins, log_psi, log_psi_fn):
    """``(spins, log_psi, basis_index)`` of a cluster as :func:`make_ising_model` takes it: the states
    sorted and unique, their log-amplitudes (given, or from ``log_psi_fn``) and, when the closure looked
    them up, their positions in the basis.  One place for :func:`make_ising_model` and
    :func:`make_ising_models`."""
    spins = np.asarray(spins, dtype=np.uint64)
    if not (spins.ndim == 1 and (spins.shape[0] < 2 or bool(np.all(spins[1:] > spins[:-1])))):
        # (the pipeline's clusters and extensions arrive sorted and unique: no sort for them)
        spins, first, multiplicity = np.unique(spins, return_index=True, return_counts=True, axis=0)
        if np.any(multiplicity != 1):
            warnings.warn("'spins' were not unique, are you sure this is what you want?")
            if log_psi is not None:
                log_psi = np.asarray(log_psi)[first]
    basis_index = None
    if log_psi is None:
        if hasattr(log_psi_fn, "index_of"):  # (ground_state_to_log_coeff_fn's closure)
            basis_index = log_psi_fn.index_of(spins)
            log_psi = log_psi_fn.at_index(basis_index)
        else:
            log_psi = log_psi_fn(spins)
    if spins.ndim > 1:
        spins = np.ascontiguousarray(spins[:, 0])
    return spins, log_psi, basis_index


def _cluster_amplitudes_and_field(hamiltonian, spins, log_psi, log_psi_fn, external_field: bool):
    """``(psi, field)`` of a cluster's Ising model from the log-amplitudes of its states: real
    amplitudes L2-normalised over the cluster (common.py:211-216) and the zero or boundary field.
    One place for :func:`make_ising_model` and :func:`reweight_ising_model`, whose models must agree
    bit for bit."""
    psi, cluster_norm = _cluster_amplitudes(log_psi)
    field = np.zeros(spins.shape[0]) if not external_field else _boundary_field(
        hamiltonian, spins, psi, log_psi_fn, cluster_norm)
    return psi, field


def _cluster_amplitudes(log_psi):
    """``(psi, cluster_norm)``: the real amplitudes of a cluster's states, L2-normalised over the cluster
    (common.py:211-216), and the norm they were divided by."""
    psi = np.exp(log_psi, dtype=np.complex128)
    if not np.allclose(psi.imag, 0, atol=1e-6):
        raise ValueError("expected all wavefunction coefficients to be real")
    psi = np.ascontiguousarray(psi.real)
    cluster_norm = norm2(psi)
    psi /= cluster_norm
    return psi, cluster_norm


def reweight_ising_model(
    model: IsingModel,
    log_psi: Optional[np.ndarray] = None,
    log_psi_fn: Optional[Callable[[np.ndarray], np.ndarray]] = None,
    external_field: bool = False,
    out: Optional[IsingModel] = None,
) -> IsingModel:
    """``make_ising_model(model.spins, model.quantum_hamiltonian, log_psi, log_psi_fn, external_field)``
    — the same states and operator, new amplitudes — for a model of one of this package's device
    operators, WITHOUT rebuilding the annealer's plan: the couplings keep their sparsity pattern as long
    as no amplitude vanishes, so the new values (``device().ising_csr``, amplitudes normalised as in
    :func:`make_ising_model`) go onto a clone of ``model``'s plan (``Hamiltonian.reweighted``), or with
    ``out=`` — a model this function returned earlier — into that model's Hamiltonian in place
    (``Hamiltonian.reweight``; a pool of clones serves a loop of any length).  ``exchange``, ``field``,
    ``initial_signs`` and every result of the returned model equal ``make_ising_model``'s bit for bit.
    When the pattern did change (``sa.PatternMismatch``), or for an operator without a device action,
    the result IS ``make_ising_model(...)`` — never an error; ``out`` is then left as it was."""
    if log_psi is None and log_psi_fn is None:
        raise ValueError("at least one of log_psi or log_psi_fn should be specified")
    if external_field and log_psi_fn is None:
        raise ValueError("log_psi_fn should be specified when external_field=True")
    operator, spins = model.quantum_hamiltonian, model.spins

    def fresh():
        return make_ising_model(spins, operator, log_psi=log_psi, log_psi_fn=log_psi_fn,
                                external_field=external_field)

    if not _on_device(operator):
        return fresh()
    basis_index = model.basis_index
    values = log_psi
    if values is None:
        if hasattr(log_psi_fn, "index_of"):
            if basis_index is None:
                basis_index = log_psi_fn.index_of(spins)
            values = log_psi_fn.at_index(basis_index)
        else:
            values = log_psi_fn(spins)
    psi, field = _cluster_amplitudes_and_field(operator, spins, values, log_psi_fn, external_field)
    try:
        indptr, col, val = operator.device().ising_csr(spins, psi)
    except _lib.AspError as error:
        if not _takes_host_route(error):
            raise
        return fresh()
    try:
        if out is not None:
            hamiltonian = out.ising_hamiltonian.reweight(val, field, indptr, col)
        else:
            hamiltonian = model.ising_hamiltonian.reweighted(val, field, indptr, col)
    except sa.PatternMismatch:
        return fresh()
    x0 = sa.signs_to_bits(np.sign(psi))
    if out is not None:
        out.initial_signs = x0
        out.basis_index = basis_index
        return out
    return IsingModel(spins, operator, hamiltonian, x0, basis_index)


def _family_stencil(model: IsingModel):
    """The coupling stencil of ``model``'s states and pattern, created on first use and kept with the
    family of its Hamiltonian (``Hamiltonian.family``: clones share it, ``release()`` of ``model``'s
    Hamiltonian closes it); ``None`` when the stencil cannot be made (one-directional matrix elements
    with duplicates: the per-model route decides what happens then)."""
    hamiltonian = model.ising_hamiltonian
    family = hamiltonian.family()
    stencil = family.get("stencil")
    exchange = hamiltonian.exchange
    if stencil is not None and family.get("pattern") is not exchange.indices:
        # (the Hamiltonian was given another matrix since: reweights keep the frozen index arrays)
        if stencil:
            stencil.release()
        stencil = None
    if stencil is None:
        try:
            stencil = model.quantum_hamiltonian.device().ising_stencil(model.spins, exchange.indptr, exchange.indices)
        except _lib.AspError as error:
            if not _takes_host_route(error):
                raise
            stencil = False  # (remembered: not tried again for every round)
        family["stencil"] = stencil
        family["pattern"] = exchange.indices
        family["owner"] = id(hamiltonian)
    return stencil or None


def reweight_ising_models(model: IsingModel, log_psis=None, log_psi_fns=None, external_field: bool = False,
                          outs=None):
    """``[reweight_ising_model(model, log_psis[d], log_psi_fns[d], external_field, outs[d]) for d in ...]``
    (not in the reference) — the same states and operator, a round of new amplitudes — with the couplings
    of ALL draws formed from the stored matrix elements of a coupling stencil (ASP-STENCIL-1, DESIGN.md
    §4.14.1) and put into the plans in ONE device call (``sa.reweight_hamiltonians``): no operator pass,
    no key lookups, no comparison of patterns per draw.  Element ``d`` equals the per-model call's bit for
    bit: ``exchange``, ``field``, ``initial_signs``, every solver result.  ``log_psis`` / ``log_psi_fns``
    / ``outs``: ``None`` or one element per draw (elements may be ``None``; every draw needs a log_psi or
    a log_psi_fn).  The stencil is created on first use and kept with the family of ``model``'s
    Hamiltonian; it goes with ``model.ising_hamiltonian.release()``.  A draw whose couplings leave the
    pattern gets ``make_ising_model``'s model; an operator without a device action, and a stencil that
    cannot be made, take the per-model route.  With ``external_field=True`` the fields of all stencil
    draws come from ONE device call (``_boundary_fields``, ASP-FIELD-SEG-1): one
    segment per draw, the same states and the same environment — computed once —, each with its own
    amplitudes and norm; every ``log_psi_fn`` is asked for the environment after the amplitudes of all
    draws are known, in draw order."""
    lengths = {len(x) for x in (log_psis, log_psi_fns, outs) if x is not None}
    if len(lengths) > 1:
        raise ValueError("'log_psis', 'log_psi_fns' and 'outs' should hold one element per draw")
    count = lengths.pop() if lengths else 0
    log_psis = [None] * count if log_psis is None else list(log_psis)
    log_psi_fns = [None] * count if log_psi_fns is None else list(log_psi_fns)
    outs = [None] * count if outs is None else list(outs)
    for log_psi, log_psi_fn in zip(log_psis, log_psi_fns):
        if log_psi is None and log_psi_fn is None:
            raise ValueError("at least one of log_psi or log_psi_fn should be specified")
        if external_field and log_psi_fn is None:
            raise ValueError("log_psi_fn should be specified when external_field=True")
    if any(a is b for k, a in enumerate(outs) if a is not None for b in outs[:k]):
        raise ValueError("'outs' holds one model twice")
    operator, spins = model.quantum_hamiltonian, model.spins

    def single(d):
        return reweight_ising_model(model, log_psis[d], log_psi_fns[d], external_field, outs[d])

    if count == 0:
        return []
    stencil = _family_stencil(model) if _on_device(operator) else None
    if stencil is None:
        return [single(d) for d in range(count)]
    base = model.ising_hamiltonian.exchange
    results = [None] * count
    draws = []  # (d, psi, field, basis_index) of the draws that go through the stencil
    for d in range(count):
        out = outs[d]
        if out is not None:
            pattern = out.ising_hamiltonian.exchange
            if not (pattern.indices is base.indices or (np.array_equal(pattern.indptr, base.indptr) and
                                                        np.array_equal(pattern.indices, base.indices))):
                results[d] = single(d)  # (a model of another pattern: the per-model call's answer)
                continue
        basis_index = model.basis_index
        values = log_psis[d]
        if values is None:
            log_psi_fn = log_psi_fns[d]
            if hasattr(log_psi_fn, "index_of"):
                if basis_index is None:
                    basis_index = log_psi_fn.index_of(spins)
                values = log_psi_fn.at_index(basis_index)
            else:
                values = log_psi_fn(spins)
        psi, cluster_norm = _cluster_amplitudes(values)
        draws.append((d, psi, cluster_norm, basis_index))
    if not draws:
        return results
    if external_field:
        # D segments of the same states and (computed once) the same environment, amplitudes per draw
        fields = _boundary_fields(operator, [(spins, psi, c) for _, psi, c, _ in draws],
                                  [log_psi_fns[d] for d, _, _, _ in draws])
    else:
        fields = [np.zeros(spins.shape[0]) for _ in draws]
    draws = [(d, psi, field, basis_index) for (d, psi, _, basis_index), field in zip(draws, fields)]
    cloned = []
    try:
        hamiltonians = []
        for d, _, _, _ in draws:
            if outs[d] is not None:
                hamiltonians.append(outs[d].ising_hamiltonian)
            else:
                cloned.append(model.ising_hamiltonian.clone())
                hamiltonians.append(cloned[-1])
        applied = sa.reweight_hamiltonians(hamiltonians, stencil, np.stack([psi for _, psi, _, _ in draws]),
                                           np.stack([field for _, _, field, _ in draws]))
    except Exception:
        for hamiltonian in cloned:
            hamiltonian.release()
        raise
    for (d, psi, _, basis_index), hamiltonian, ok in zip(draws, hamiltonians, applied):
        if not ok:
            if outs[d] is None:
                hamiltonian.release()
            results[d] = make_ising_model(spins, operator, log_psi=log_psis[d], log_psi_fn=log_psi_fns[d],
                                          external_field=external_field)
            continue
        x0 = sa.signs_to_bits(np.sign(psi))
        if outs[d] is not None:
            outs[d].initial_signs = x0
            outs[d].basis_index = basis_index
            results[d] = outs[d]
        else:
            results[d] = IsingModel(spins, operator, hamiltonian, x0, basis_index)
    return results


def _boundary_field(hamiltonian, spins, psi, log_psi_fn, cluster_norm: float) -> np.ndarray:
    """The field of ``make_ising_model(..., external_field=True)``: the environment is the one-hop
    extension of the cluster, its signed amplitudes come from ``log_psi_fn`` in the cluster's
    normalisation, and ``scale = 2`` (ASP-FIELD-1)."""
    env_keys = extension_spins(hamiltonian, spins)
    if hasattr(log_psi_fn, "index_of"):  # (ground_state_to_log_coeff_fn's closure)
        env_log_psi = log_psi_fn.at_index(log_psi_fn.index_of(env_keys))
    else:
        env_log_psi = log_psi_fn(env_keys)
    env_psi = np.exp(env_log_psi, dtype=np.complex128)
    if not np.allclose(env_psi.imag, 0, atol=1e-6):
        raise ValueError("expected all wavefunction coefficients to be real")
    env_psi = np.ascontiguousarray(env_psi.real)
    env_psi /= cluster_norm
    field, unresolved = hamiltonian.device().field(spins, psi, env_keys, env_psi, scale=2.0)
    if unresolved > 0:
        raise ValueError("{} connections leave the cluster for states outside its environment".format(unresolved))
    return field


def _boundary_fields(hamiltonian, clusters, log_psi_fns) -> list:
    """``[_boundary_field(hamiltonian, spins, psi, log_psi_fn, cluster_norm) for spins, psi, cluster_norm in
    clusters]`` for prepared clusters of ONE device operator, with all environments from one
    :func:`extension_spins_segments` call and all fields from one ``DeviceOperator.field_segments`` call
    (ASP-FIELD-SEG-1): the same fields bit for bit.  ``log_psi_fns``: one callable for
    all clusters, or one per cluster.  Clusters that share their ``spins`` array (the draws of a noise
    study) share one environment, which is computed once.  The amplitude lookups are the loop's — per
    cluster, in cluster order, with the arguments the loop passes —; only their interleaving with whatever
    the caller does between the clusters changes, so a pure ``log_psi_fn`` gives identical fields.  The
    ``ValueError`` for connections that leave a cluster's environment is that of the FIRST such cluster,
    the one the loop raises.  A call refused for its size (ASP_ERR_TOO_LARGE), or in a way after which
    the host route does the job, takes the loop."""
    clusters = list(clusters)
    if not clusters:
        return []
    if callable(log_psi_fns):
        log_psi_fns = [log_psi_fns] * len(clusters)

    def loop():
        return [_boundary_field(hamiltonian, spins, psi, fn, cluster_norm)
                for (spins, psi, cluster_norm), fn in zip(clusters, log_psi_fns)]

    distinct, key_sets = {}, []  # id(spins) -> position among the distinct key sets
    for spins, _, _ in clusters:
        if id(spins) not in distinct:
            distinct[id(spins)] = len(key_sets)
            key_sets.append(spins)
    try:
        extended = extension_spins_segments(hamiltonian, key_sets)
    except _lib.AspError as error:
        if not (error.code == -4 or _takes_host_route(error)):
            raise
        return loop()
    environments = []
    for (spins, _, cluster_norm), log_psi_fn in zip(clusters, log_psi_fns):
        env_keys = extended[distinct[id(spins)]]
        if hasattr(log_psi_fn, "index_of"):  # (ground_state_to_log_coeff_fn's closure)
            env_log_psi = log_psi_fn.at_index(log_psi_fn.index_of(env_keys))
        else:
            env_log_psi = log_psi_fn(env_keys)
        env_psi = np.exp(env_log_psi, dtype=np.complex128)
        if not np.allclose(env_psi.imag, 0, atol=1e-6):
            raise ValueError("expected all wavefunction coefficients to be real")
        env_psi = np.ascontiguousarray(env_psi.real)
        env_psi /= cluster_norm
        environments.append((env_keys, env_psi))
    offsets = np.zeros(len(clusters) + 1, dtype=np.uint64)
    np.cumsum([spins.shape[0] for spins, _, _ in clusters], out=offsets[1:])
    env_offsets = np.zeros(len(clusters) + 1, dtype=np.uint64)
    np.cumsum([env_keys.shape[0] for env_keys, _ in environments], out=env_offsets[1:])
    try:
        field, unresolved = hamiltonian.device().field_segments(
            np.concatenate([spins for spins, _, _ in clusters]), np.concatenate([psi for _, psi, _ in clusters]),
            offsets, np.concatenate([env_keys for env_keys, _ in environments]),
            np.concatenate([env_psi for _, env_psi in environments]), env_offsets, scale=2.0)
    except _lib.AspError as error:
        if not (error.code == -4 or _takes_host_route(error)):
            raise
        return loop()
    lost = np.flatnonzero(unresolved)
    if lost.size:
        raise ValueError("{} connections leave the cluster for states outside its environment".format(
            int(unresolved[lost[0]])))
    return [field[int(offsets[g]):int(offsets[g + 1])].copy() for g in range(len(clusters))]


def compute_accuracy_and_overlap(
    predicted: np.ndarray,
    exact: np.ndarray,
    weights: Optional[np.ndarray] = None,
    number_spins: Optional[int] = None,
) -> Tuple[float, float]:
    """Sign accuracy and weighted overlap, both invariant under a global flip
    (common.py:211-229)."""
    if weights is None and number_spins is None:
        raise ValueError("'weights' and 'number_spins' cannot be both None")
    if number_spins is None:
        number_spins = len(weights)
    if weights is None:
        weights = np.ones(number_spins, dtype=np.float64)
    guess = sa.bits_to_signs(predicted, number_spins)
    truth = sa.bits_to_signs(exact, number_spins)
    accuracy = np.mean(truth == guess)
    accuracy = max(accuracy, 1 - accuracy)
    overlap = abs(np.dot(truth * guess, weights / np.sum(weights)))
    return accuracy, overlap


def compute_accuracies_and_overlaps(predicted_list, exact_list, weights_list) -> list:
    """``[compute_accuracy_and_overlap(p, e, w) for p, e, w in zip(...)]`` as ONE device call
    (``scores.accuracy_and_overlap_each``: ``asp_sign_scores_batch``, specification ASP-SCORE-1,
    DESIGN.md §3.11): a list of ``(accuracy, overlap)``.  Every accuracy is the host function's bit for
    bit; every overlap is within ``(K + 64) * 2**-53`` of it (a pairwise tree instead of a dot product
    with the normalised weights)."""
    from . import scores

    accuracy, overlap = scores.accuracy_and_overlap_each(list(predicted_list), list(exact_list), list(weights_list))
    return list(zip(accuracy, overlap))


def binary_search(haystack, needles) -> np.ndarray:
    """Positions of ``needles`` in sorted ``haystack``; all must be present
    (common.py:544-548)."""
    haystack = np.asarray(haystack)
    needles = np.asarray(needles)
    assert haystack.shape[0] < 2 or np.all(haystack[1:] >= haystack[:-1])  # (sorted)
    indices = np.searchsorted(haystack, needles)
    assert np.all(haystack[np.minimum(indices, haystack.shape[0] - 1)] == needles)
    return indices


def solve_ising_model(
    model: IsingModel,
    mode: str = "sa",
    frozen_spins: Optional[np.ndarray] = None,
    seed: int = 12345,
    number_sweeps: int = 5120,
    repetitions: int = 64,
    only_best: bool = True,
    sweep_order: Optional[str] = None,
    select: str = "best",
    tree: Optional[str] = None,
) -> np.ndarray:
    """Optimise the signs of ``model`` and project them onto ``frozen_spins``
    (common.py:232-261).  ``sweep_order`` (not in the reference): ``"shuffled"``, a fresh random
    order every sweep as in the reference's annealer — the default, so that the drop-in call has
    the reference's law —, or ``"colour"``, this package's fixed colour order (faster, a different
    chain; ``sa.anneal``); ``None`` = ``$ASP_SWEEP_ORDER`` or shuffled.
    ``tree`` (not in the reference; ``mode="greedy"``): ``"host"`` or ``"device"``, where the greedy
    solver's strongest-coupling tree is built; ``None`` = ``$ASP_GREEDY_TREE`` or host.  The same signs.
    ``select`` (not in the reference; ``mode="sa"``): ``"best"``, the chain of lowest energy, or
    ``"consensus"``, the vote of all chains (:func:`_consensus_of_chains`)."""
    _check_select(select, mode, "anneal", None)
    if mode == "sa" and select == "consensus":
        xs, es = sa.anneal(model.ising_hamiltonian, seed=seed, number_sweeps=number_sweeps,
                           repetitions=repetitions, only_best=False, sweep_order=sweep_order)
        x = _consensus_of_chains([model], [(xs, es)])[0]
    elif mode == "sa":
        x, _ = sa.anneal(model.ising_hamiltonian, seed=seed, number_sweeps=number_sweeps,
                         repetitions=repetitions, only_best=only_best, sweep_order=sweep_order)
    elif mode == "greedy":
        x, _ = sa.greedy_solve(model.ising_hamiltonian, tree=tree)
    else:
        raise ValueError(
            "invalid mode specified: '{}'; expected either 'sa' or 'greedy'".format(mode))
    return _project_on_frozen(model, x, frozen_spins)


def _check_select(select: str, mode: str, method: str, patience) -> None:
    if select not in ("best", "consensus"):
        raise ValueError("invalid select specified: '{}'; expected 'best' or 'consensus'".format(select))
    if select == "consensus" and (mode != "sa" or method != "anneal" or patience is not None):
        raise ValueError("select='consensus' votes over the chains of a plain anneal: it needs mode='sa' and "
                         "method='anneal', without 'patience'")


def _consensus_of_chains(models, chains) -> list:
    """The consensus configuration of every model's chains ``(xs[R, words], es[R])`` — the uniform vote
    of law ASP-VOTE-1, anchored on the first chain of lowest energy and aligned up to
    the global flip exactly when the model has no field — for ALL models in one device call
    (``scores.consensus_batch``)."""
    from . import scores

    items = [dict(xs=xs, number_spins=m.ising_hamiltonian.size, anchor=int(np.argmin(es)),
                  align=not np.any(m.ising_hamiltonian.field)) for m, (xs, es) in zip(models, chains)]
    return [c.x for c in scores.consensus_batch(items)]


def _project_on_frozen(model: IsingModel, x: np.ndarray, frozen_spins) -> np.ndarray:
    """The signs of ``frozen_spins`` out of a solution of ``model`` (common.py:256-260)."""
    if frozen_spins is None:
        return x
    where = binary_search(model.spins, frozen_spins)
    signs = sa.bits_to_signs(x, count=model.spins.size)
    return sa.signs_to_bits(signs[where])


def solve_ising_models(models, frozen_spins=None, seed: int = 12345, number_sweeps: int = 5120,
                       repetitions: int = 64, sweep_order: Optional[str] = None, mode: str = "sa",
                       check_every: Optional[int] = None, patience: Optional[int] = None,
                       method: str = "anneal", plan_batch: bool = False, select: str = "best",
                       tree: Optional[str] = None):
    """``[solve_ising_model(m, mode, f, seed, number_sweeps, repetitions) for m, f in
    zip(models, frozen_spins)]`` with all annealing chains of all models in ONE device call
    (``sa.anneal_batch``): the same result for every model, at the throughput of a full chip
    instead of one small launch per model.  ``mode="greedy"``: the greedy solves of all models in
    one call (``sa.greedy_solve_batch``), with the same projection on the frozen spins.
    ``patience`` (not in the reference; default off): every model's ladder runs in segments of
    ``check_every`` sweeps (default 512) and stops once none of its chains improved for ``patience``
    consecutive segments (``sa.anneal_batch_until``) — fewer sweeps, results that may differ.
    ``method`` (not in the reference; default ``"anneal"``): ``"population"``, ``"tempering"`` or
    ``"tempering-cluster"`` solve every model with ``sa.population_anneal_batch`` /
    ``sa.parallel_tempering_batch`` / ``sa.parallel_tempering_cluster_batch`` (isoenergetic cluster moves
    in every round; an even ``repetitions``) instead, in ``number_sweeps // 10`` steps / rounds of ten
    sweeps — the sweep count of the plain call.
    ``tree`` (``mode="greedy"``): as in :func:`solve_ising_model`.
    ``plan_batch`` (not in the reference; default off): the sweep plans of all models are made by one
    segmented device call (``sa.plan_hamiltonians``) before the solve instead of one by one inside it;
    the results are the same.
    ``select`` (not in the reference; default ``"best"``): ``"consensus"`` returns, instead of every
    model's chain of lowest energy, the vote of all its chains — uniform weights, anchored on that
    chain, aligned up to the global flip where the model has no field (law ASP-VOTE-1, DESIGN.md
    §3.12) —, all models in one ``scores.consensus_batch`` call; plain anneals only."""
    if method not in ("anneal", "population", "tempering", "tempering-cluster"):
        raise ValueError("invalid method specified: '{}'; expected 'anneal', 'population', 'tempering' or "
                         "'tempering-cluster'".format(method))
    if method != "anneal":
        if mode != "sa":
            raise ValueError("'method' selects an annealing method: it needs mode='sa'")
        if patience is not None:
            raise ValueError("method='{}' cannot be combined with 'patience'".format(method))
        if int(number_sweeps) < 10:
            raise ValueError("method='{}' runs steps of ten sweeps: 'number_sweeps' must be at least 10".format(method))
    _check_select(select, mode, method, patience)
    models = list(models)
    frozen = [None] * len(models) if frozen_spins is None else list(frozen_spins)
    if mode not in ("sa", "greedy"):
        raise ValueError(
            "invalid mode specified: '{}'; expected either 'sa' or 'greedy'".format(mode))
    if plan_batch:
        sa.plan_hamiltonians([m.ising_hamiltonian for m in models])
    if mode == "greedy":
        solved = sa.greedy_solve_batch([m.ising_hamiltonian for m in models], tree=tree)
        return [_project_on_frozen(m, x, f) for m, (x, _), f in zip(models, solved, frozen)]
    if mode != "sa":
        raise ValueError(
            "invalid mode specified: '{}'; expected either 'sa' or 'greedy'".format(mode))
    if method != "anneal":
        hamiltonians = [m.ising_hamiltonian for m in models]
        steps = int(number_sweeps) // 10
        if method == "population":
            best = sa.population_anneal_batch(hamiltonians, seed=seed, number_steps=steps, sweeps_per_step=10,
                                              repetitions=repetitions, only_best=True, sweep_order=sweep_order)
        elif method == "tempering":
            best = sa.parallel_tempering_batch(hamiltonians, seed=seed, number_rounds=steps, sweeps_per_round=10,
                                               repetitions=repetitions, only_best=True, sweep_order=sweep_order)
        else:
            best = sa.parallel_tempering_cluster_batch(hamiltonians, seed=seed, number_rounds=steps,
                                                       sweeps_per_round=10, repetitions=repetitions, only_best=True,
                                                       sweep_order=sweep_order)
        return [_project_on_frozen(m, x, f) for m, (x, _), f in zip(models, best, frozen)]
    if patience is not None:
        best = sa.anneal_batch_until([m.ising_hamiltonian for m in models], seed=seed,
                                     number_sweeps=number_sweeps, repetitions=repetitions, only_best=True,
                                     sweep_order=sweep_order, patience=patience,
                                     check_every=512 if check_every is None else check_every)
        return [_project_on_frozen(m, x, f) for m, (x, _, _), f in zip(models, best, frozen)]
    if select == "consensus":
        chains = sa.anneal_batch([m.ising_hamiltonian for m in models], seed=seed, number_sweeps=number_sweeps,
                                 repetitions=repetitions, only_best=False, sweep_order=sweep_order)
        voted = _consensus_of_chains(models, chains)
        return [_project_on_frozen(m, x, f) for m, x, f in zip(models, voted, frozen)]
    best = sa.anneal_batch([m.ising_hamiltonian for m in models], seed=seed,
                           number_sweeps=number_sweeps, repetitions=repetitions, only_best=True,
                           sweep_order=sweep_order)
    return [_project_on_frozen(m, x, f) for m, (x, _), f in zip(models, best, frozen)]


def make_hamiltonian_extension(model: IsingModel, log_psi_fn, external_field: bool = False) -> IsingModel:
    """One-hop extension of a cluster: every state connected to it (common.py:516-522).
    ``external_field`` (not in the reference): passed on to :func:`make_ising_model`."""
    spins = extension_spins(model.quantum_hamiltonian, model.spins)
    if not external_field:
        return make_ising_model(spins, model.quantum_hamiltonian, log_psi_fn=log_psi_fn)
    return make_ising_model(spins, model.quantum_hamiltonian, log_psi_fn=log_psi_fn, external_field=True)


def extension_spins(hamiltonian, spins) -> np.ndarray:
    """The sorted unique states connected to ``spins`` (their own included).  In a symmetry sector
    with a character -1 a connection can point at an orbit of norm 0: its coefficient is exactly 0
    and it is no basis state, so it is left out (on the device: asp_operator_extend)."""
    if _on_device(hamiltonian):
        return hamiltonian.device().extend(spins)  # sorted and unique
    other, _, _ = _batched_apply(hamiltonian, spins)
    other = np.unique(other, axis=0)
    group = getattr(hamiltonian.basis, "group", None)
    if group is not None and getattr(group, "spin_inversion", 0) < 0:
        other = other[group.state_info(other)[2] > 0]
    return other


def local_energies(hamiltonian, spins, signed_psi, rows=None):
    """``(hphi, eloc, missing)`` of the state with the signed amplitudes ``signed_psi`` (any
    normalisation) on the ascending unique states ``spins``, specification ASP-ELOC-1 (DESIGN.md
    §3.7): ``hphi[r] = sum_s' H_ss' psi_s'`` over the connections of row r that stay inside
    ``spins``, ``eloc[r] = hphi[r] / psi_r`` and the number of connections with a non-zero matrix
    element that leave ``spins`` (they contribute nothing).  ``rows``: positions in ``spins``, any
    order, repeats allowed; ``None``: every state.  Not in the reference, whose local energy
    (experiments/sampled_connected_components.py:294-312) loops over the connections in Python;
    this package's device operators only."""
    if not _on_device(hamiltonian):
        raise NotImplementedError(
            "local energies need one of this package's device operators (operators.Operator with real "
            "matrices); they are not implemented for foreign operator objects")
    spins = np.asarray(spins, dtype=np.uint64)
    if spins.ndim > 1:
        spins = np.ascontiguousarray(spins[:, 0])
    return hamiltonian.device().local_energy(spins, signed_psi, None, rows)


def variational_energy(hamiltonian, spins, signed_psi) -> Tuple[float, int]:
    """``(energy, missing_total)``: the Rayleigh quotient ``sum_r psi_r (H psi)_r / sum_r psi_r^2`` of
    the state with the signed amplitudes ``signed_psi`` on ``spins``, from :func:`local_energies`
    (``H`` restricted to ``spins``), and the number of connections that leave ``spins``.  Over a full
    basis that number is 0 and the energy is ``Operator.expectation``."""
    if not _on_device(hamiltonian):
        raise NotImplementedError(
            "the variational energy needs one of this package's device operators (operators.Operator with "
            "real matrices); it is not implemented for foreign operator objects")
    signed_psi = np.ascontiguousarray(signed_psi, dtype=np.float64)
    spins = np.asarray(spins, dtype=np.uint64)
    if spins.ndim > 1:
        spins = np.ascontiguousarray(spins[:, 0])
    # (no quotient per row: a state of amplitude zero is legal here)
    hphi, _, missing = hamiltonian.device()._local_energy(spins, signed_psi, None, None, False)
    return dot(signed_psi, hphi) / dot(signed_psi, signed_psi), int(missing.sum(dtype=np.int64))


def get_strongest_off_diag(matrix) -> np.ndarray:
    """Per row, the largest |J_ij| with j != i (common.py:525-541)."""
    m = scipy.sparse.csr_matrix(matrix)
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    magnitude = np.where(rows != m.indices, np.abs(m.data), 0.0)
    out = np.zeros(m.shape[0], dtype=m.data.dtype)
    np.maximum.at(out, rows, magnitude)
    return out


def cluster_statistics(spins, quantum_hamiltonian, ground_state) -> dict:
    """``{"spins", "bonds", "frustrated", "largest_frustrated"}`` of the Ising model of a cluster
    with the ground state's own signs — the four numbers common.py:439-478 logs: the number of bonds
    (off-diagonal non-zeros, both directions), the fraction of them that is frustrated
    (``J_ij s_i s_j > 0``) and the fraction of spins whose strongest bond is.  One deliberate
    difference: the reference takes ``argmax`` of the SIGNED matrix with its implicit zeros (it
    computes ``positive_matrix`` and never uses it); here the strongest bond is the one of largest
    magnitude, the smallest column on a tie."""
    from .bonds import BondStatistics

    log_psi_fn = ground_state_to_log_coeff_fn(ground_state, quantum_hamiltonian.basis)
    model = make_ising_model(spins, quantum_hamiltonian, log_psi_fn=log_psi_fn)
    with BondStatistics(model.ising_hamiltonian, model.initial_signs) as stats:
        summary = stats.summary
    size, bonds = model.size, summary["bonds"]
    return {"spins": size, "bonds": bonds,
            "frustrated": summary["frustrated"] / bonds if bonds else float("nan"),
            "largest_frustrated": summary["strongest_frustrated"] / size if size else float("nan")}


def coupling_distribution(model: IsingModel) -> np.ndarray:
    """``|J_ij|`` of all bonds of the model in descending order (common.py:955-959), sorted on the
    device."""
    from .bonds import BondStatistics

    with BondStatistics(model.ising_hamiltonian, model.initial_signs) as stats:
        return stats.magnitudes()


def probability_of_frustration(model, signs=None, bins: int = 50, span: float = 20.0, min_count: int = 100):
    """``(x, y, normal, frustrated)``: the probability ``y`` that a bond of strength ``x`` is NOT
    frustrated (common.py:977-1001).  ``bins`` log-space edges from ``lo = max(log max|J| - span,
    log min|J|)`` to ``log max|J|``; ``normal`` and ``frustrated`` are the counts of the ``bins - 1``
    bins, ``y = normal / (normal + frustrated)`` with NaN where the total is below ``min_count``, and
    ``x = exp`` of the bin centres.  ``signs``: packed sign bits, by default ``model.initial_signs``.
    ``model`` may also be a :class:`.bonds.BondStatistics` (its signs are used unless given)."""
    from .bonds import BondStatistics, log_edges

    bins = int(bins)
    if bins < 2:
        raise ValueError("'bins' counts the edges: at least 2")
    owned = not isinstance(model, BondStatistics)
    stats = BondStatistics(model.ising_hamiltonian, model.initial_signs if signs is None else signs) if owned else model
    try:
        if not owned and signs is not None:
            stats.set_signs(signs)
        summary = stats.summary
        if summary["bonds"] == 0:
            raise ValueError("the model has no bonds")
        hi = np.log(summary["max_abs"])
        lo = max(hi - span, np.log(summary["min_abs"]))
        if not lo < hi:
            raise ValueError("all bonds have the same strength: there is nothing to bin")
        normal, frustrated, _, _ = stats.histogram(log_edges(lo, hi, bins))
    finally:
        if owned:
            stats.release()
    log_bins = np.linspace(lo, hi, bins)
    total = normal + frustrated
    with np.errstate(divide="ignore", invalid="ignore"):
        y = normal / total
    y[total < min_count] = float("nan")
    x = np.exp(0.5 * (log_bins[:-1] + log_bins[1:]))
    return x, y, normal, frustrated


def sparsify_component(exchange, is_frozen, reltol: float, anchor: int):
    """``(keep bool[K], block csr_matrix)`` through ``asp_sparsify_component``: cutoff, component
    of ``anchor`` and the un-pruned block on it, all on the GPU (csrc/sparsify.hip)."""
    lib = _lib.load()
    _lib.require_gpu()
    full = scipy.sparse.csr_matrix(exchange)
    if not full.has_sorted_indices:
        full = full.sorted_indices()
    full.sum_duplicates()
    k = full.shape[0]
    indptr = np.ascontiguousarray(full.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(full.indices, dtype=np.int32)
    data = np.ascontiguousarray(full.data, dtype=np.float64)
    frozen = np.ascontiguousarray(is_frozen, dtype=np.uint8)
    keep = np.zeros(max(k, 1), dtype=np.uint8)
    kept, nnz = ctypes.c_uint64(0), ctypes.c_uint64(0)
    capacity = int(data.shape[0])
    out_indptr = np.zeros(k + 1, dtype=np.int64)
    out_indices = np.empty(max(capacity, 1), dtype=np.int32)
    out_data = np.empty(max(capacity, 1), dtype=np.float64)
    _lib.check(lib.asp_sparsify_component(
        ctypes.c_uint64(k), _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data), _lib.ptr(frozen),
        ctypes.c_double(float(reltol)), ctypes.c_uint64(int(anchor)), _lib.ptr(keep),
        ctypes.byref(kept), ctypes.c_uint64(capacity), _lib.ptr(out_indptr), _lib.ptr(out_indices),
        _lib.ptr(out_data), ctypes.byref(nnz)))
    n, z = int(kept.value), int(nnz.value)
    block = scipy.sparse.csr_matrix((out_data[:z].copy(), out_indices[:z].copy(),
                                     out_indptr[:n + 1].astype(np.int32)), shape=(n, n))
    block.has_sorted_indices = True  # (rows of a canonical matrix restricted to a subset)
    block.has_canonical_format = True
    return keep[:k].astype(bool), block


def sparsify_using_global_cutoff(model: IsingModel, reltol: float, frozen_spins) -> IsingModel:
    """Drop couplings below ``reltol * max|J|`` (unless both ends are frozen) and keep
    the connected component that holds the frozen spins (common.py:634-692)."""
    frozen = binary_search(model.spins, frozen_spins)
    is_frozen = np.zeros(model.spins.shape[0], dtype=bool)
    is_frozen[frozen] = True
    # NB: like the reference (common.py:674) the kept block comes from the UN-pruned matrix:
    # the cutoff only decides which spins survive.
    keep, exchange = sparsify_component(model.ising_hamiltonian.exchange, is_frozen, reltol,
                                        int(frozen[0]))
    spins = model.spins[keep]
    signs = sa.bits_to_signs(model.initial_signs, model.size)[keep]
    field = model.ising_hamiltonian.field[keep]
    hamiltonian = sa.Hamiltonian.from_canonical_csr(exchange.indptr, exchange.indices, exchange.data, field)
    basis_index = None if model.basis_index is None else model.basis_index[keep]
    return IsingModel(spins, model.quantum_hamiltonian, hamiltonian, sa.signs_to_bits(signs), basis_index)


def sparsify_component_segments(offsets, indptr, indices, data, is_frozen, reltol: float, anchors):
    """:func:`sparsify_component` of many matrices in one device call, specification ASP-SPARSIFY-SEG-1
    (csrc/level_segments.hip).  The input is laid out as ``DeviceOperator.ising_csr_segments``
    returns it: ``offsets`` u64[G + 1] cuts the T spins into segments, ``indptr`` is ONE global i64[T + 1]
    from 0, ``indices`` are local to their segment; ``is_frozen`` bool[T]; ``anchors`` u64[G], local.
    Returns ``(keep bool[T], kept_offsets u64[G + 1], out_indptr i64[kept + 1], out_indices i32, out_data
    f64)`` in the same layout over the kept spins; the threshold is ``reltol * max|data|`` of each segment."""
    lib = _lib.load()
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    frozen = np.ascontiguousarray(is_frozen, dtype=np.uint8)
    anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
    if offsets.ndim != 1 or offsets.shape[0] < 1:
        raise ValueError("offsets should hold one entry more than there are segments")
    segments = offsets.shape[0] - 1
    t = int(offsets[-1])
    if indptr.shape != (t + 1,) or frozen.shape != (t,) or anchors.shape != (segments,):
        raise ValueError("indptr, is_frozen and anchors should have T + 1, T and G entries")
    if indices.shape != data.shape or indices.shape[0] < int(indptr[-1]):
        raise ValueError("indices and data should hold indptr[-1] entries")
    if t > 0:
        _lib.require_gpu()
    keep = np.zeros(max(t, 1), dtype=np.uint8)
    kept_offsets = np.zeros(segments + 1, dtype=np.uint64)
    capacity = int(indptr[-1])
    out_indptr = np.zeros(t + 1, dtype=np.int64)
    out_indices = np.empty(max(capacity, 1), dtype=np.int32)
    out_data = np.empty(max(capacity, 1), dtype=np.float64)
    nnz = ctypes.c_uint64(0)
    _lib.check(lib.asp_sparsify_component_segments(
        ctypes.c_uint64(segments), _lib.ptr(offsets), _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
        _lib.ptr(frozen), ctypes.c_double(float(reltol)), _lib.ptr(anchors), _lib.ptr(keep), _lib.ptr(kept_offsets),
        ctypes.c_uint64(capacity), _lib.ptr(out_indptr), _lib.ptr(out_indices), _lib.ptr(out_data),
        ctypes.byref(nnz)))
    n, z = int(kept_offsets[-1]), int(nnz.value)
    return keep[:t].astype(bool), kept_offsets, out_indptr[:n + 1], out_indices[:z], out_data[:z]


def sparsify_models_using_global_cutoff(models, reltol: float, frozen_spins_list):
    """``[sparsify_using_global_cutoff(m, reltol, f) for m, f in zip(models, frozen_spins_list)]`` (not in
    the reference) with the cutoff, the components and the kept blocks of ALL models from one device call
    (:func:`sparsify_component_segments`): the same models field by field.  The models' CSR arrays are
    concatenated as they are — no scipy matrix is built per cluster on the way in."""
    models = list(models)
    frozen_spins_list = list(frozen_spins_list)
    if len(frozen_spins_list) != len(models):
        raise ValueError("'frozen_spins_list' should hold one array per model")
    if not models:
        return []
    offsets = np.zeros(len(models) + 1, dtype=np.uint64)
    np.cumsum([m.spins.shape[0] for m in models], out=offsets[1:])
    total = int(offsets[-1])
    is_frozen = np.zeros(total, dtype=bool)
    anchors = np.zeros(len(models), dtype=np.uint64)
    indptr = np.zeros(total + 1, dtype=np.int64)
    base = 0
    for g, (model, frozen_spins) in enumerate(zip(models, frozen_spins_list)):
        first, last = int(offsets[g]), int(offsets[g + 1])
        frozen = binary_search(model.spins, frozen_spins)
        is_frozen[first:last][frozen] = True
        anchors[g] = int(frozen[0])
        own = model.ising_hamiltonian.exchange.indptr
        indptr[first + 1:last + 1] = own[1:].astype(np.int64) + base
        base += int(own[-1])
    indices = np.concatenate([m.ising_hamiltonian.exchange.indices for m in models])
    data = np.concatenate([m.ising_hamiltonian.exchange.data for m in models])
    keep, kept_offsets, out_indptr, out_indices, out_data = sparsify_component_segments(
        offsets, indptr, indices, data, is_frozen, reltol, anchors)
    out = []
    for g, model in enumerate(models):
        mask = keep[int(offsets[g]):int(offsets[g + 1])]
        first, last = int(kept_offsets[g]), int(kept_offsets[g + 1])
        begin, end = int(out_indptr[first]), int(out_indptr[last])
        signs = sa.bits_to_signs(model.initial_signs, model.size)[mask]
        hamiltonian = sa.Hamiltonian.from_canonical_csr(
            (out_indptr[first:last + 1] - begin).astype(np.int32), out_indices[begin:end].copy(),
            out_data[begin:end].copy(), model.ising_hamiltonian.field[mask])
        basis_index = None if model.basis_index is None else model.basis_index[mask]
        out.append(IsingModel(model.spins[mask], model.quantum_hamiltonian, hamiltonian, sa.signs_to_bits(signs),
                              basis_index))
    return out


def extension_spins_segments(hamiltonian, spins_list) -> list:
    """``[extension_spins(hamiltonian, s) for s in spins_list]`` (not in the reference) with the
    extensions of ALL sets from one device call (``DeviceOperator.extend_segments``, ASP-EXTEND-SEG-1,
    DESIGN.md §3.10).  Foreign operator objects take that loop."""
    spins_list = list(spins_list)
    if not _on_device(hamiltonian) or not spins_list:
        return [extension_spins(hamiltonian, s) for s in spins_list]
    parts = [np.ascontiguousarray(s, dtype=np.uint64) for s in spins_list]
    offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([p.shape[0] for p in parts], out=offsets[1:])
    states, out_offsets = hamiltonian.device().extend_segments(np.concatenate(parts), offsets)
    return [states[int(out_offsets[g]):int(out_offsets[g + 1])].copy() for g in range(len(parts))]


def extend_and_sparsify_models(models, log_psi_fn, reltol: float, frozen_spins_list, external_field: bool = False):
    """One level of a round in three steps (not in the reference): :func:`extension_spins_segments` ->
    :func:`make_ising_models` -> :func:`sparsify_models_using_global_cutoff`, each ONE device call for all
    clusters.  Equals ``[sparsify_using_global_cutoff(make_hamiltonian_extension(m, log_psi_fn,
    external_field), reltol, f) for m, f in zip(models, frozen_spins_list)]`` field by field; models of
    different operators take that loop."""
    models = list(models)
    frozen_spins_list = list(frozen_spins_list)
    if len(frozen_spins_list) != len(models):
        raise ValueError("'frozen_spins_list' should hold one array per model")
    if not models:
        return []
    operator = models[0].quantum_hamiltonian
    if any(m.quantum_hamiltonian is not operator for m in models):
        return [sparsify_using_global_cutoff(make_hamiltonian_extension(m, log_psi_fn, external_field), reltol, f)
                for m, f in zip(models, frozen_spins_list)]
    extended = extension_spins_segments(operator, [m.spins for m in models])
    built = make_ising_models(extended, operator, log_psi_fn=log_psi_fn, external_field=external_field)
    return sparsify_models_using_global_cutoff(built, reltol, frozen_spins_list)


def invert_permutation(p) -> np.ndarray:
    """``s`` with ``s[p[i]] = i`` (common.py:110-113)."""
    p = np.asarray(p)
    s = np.empty_like(p)
    s[p] = np.arange(p.size)
    return s


def _h5py_or_none():
    try:
        import h5py  # optional: not part of this image's main interpreter

        return h5py
    except Exception:
        return None


def dump_ising_model_to_hdf5(model: IsingModel, ground_state, filename: str) -> None:
    """The reference's dump of an Ising model (common.py:750-769), same dataset names, dtypes and
    layout: ``elements f64[nnz]``, ``indices i32[nnz]``, ``indptr i32[K+1]`` (CSR of J),
    ``field f64[K]``, ``energy`` (<psi|H|psi>, scalar f64) and ``signs u64[ceil(K/64)]`` at the
    root.  Written with h5py when it is importable, otherwise with :mod:`.hdf5_lite`."""
    matrix = scipy.sparse.csr_matrix(model.ising_hamiltonian.exchange)
    ground_state = np.asarray(ground_state, dtype=np.float64)
    energy = float(np.real(model.quantum_hamiltonian.expectation(ground_state)))
    content = {
        "elements": np.asarray(matrix.data, dtype=np.float64),
        "indices": np.asarray(matrix.indices, dtype=np.int32),
        "indptr": np.asarray(matrix.indptr, dtype=np.int32),
        "field": np.asarray(model.ising_hamiltonian.field, dtype=np.float64),
        "energy": np.float64(energy),
        "signs": sa.signs_to_bits(np.sign(ground_state)),
    }
    h5py = _h5py_or_none()
    if h5py is not None:
        with h5py.File(filename, "w") as out:
            for key, value in content.items():
                out[key] = value
        return
    from . import hdf5_lite

    hdf5_lite.write(filename, content)


def load_ising_model_from_hdf5(filename: str):
    """Inverse of :func:`dump_ising_model_to_hdf5`: ``(Hamiltonian, energy, signs)``."""
    h5py = _h5py_or_none()
    if h5py is not None:
        with h5py.File(filename, "r") as f:
            c = {k: np.asarray(f[k]) for k in ("elements", "indices", "indptr", "field", "energy", "signs")}
    else:
        from . import hdf5_lite

        c = hdf5_lite.read(filename)
    n = c["field"].shape[0]
    exchange = scipy.sparse.csr_matrix(
        (np.asarray(c["elements"], dtype=np.float64), np.asarray(c["indices"], dtype=np.int32),
         np.asarray(c["indptr"], dtype=np.int32)), shape=(n, n))
    return (sa.Hamiltonian(exchange, np.asarray(c["field"], dtype=np.float64)), float(c["energy"]),
            np.asarray(c["signs"], dtype=np.uint64))


def load_ground_state(filename: str):
    """``(ground_state f64[N], energy, basis_representatives u64[N])`` of a SpinED output file
    (common.py:772-780): ``/hamiltonian/eigenvectors`` (first vector), ``/hamiltonian/eigenvalues``
    and ``/basis/representatives``."""
    h5py = _h5py_or_none()
    if h5py is not None:
        with h5py.File(filename, "r") as f:
            vectors = np.asarray(f["/hamiltonian/eigenvectors"], dtype=np.float64)
            values = np.asarray(f["/hamiltonian/eigenvalues"], dtype=np.float64)
            representatives = np.asarray(f["/basis/representatives"], dtype=np.uint64)
    else:
        from . import hdf5_lite

        tree = hdf5_lite.read(filename)
        vectors = np.asarray(hdf5_lite.lookup(tree, "/hamiltonian/eigenvectors"), dtype=np.float64)
        values = np.asarray(hdf5_lite.lookup(tree, "/hamiltonian/eigenvalues"), dtype=np.float64)
        representatives = np.asarray(hdf5_lite.lookup(tree, "/basis/representatives"), dtype=np.uint64)
    ground_state = vectors.squeeze()
    if ground_state.ndim > 1:
        ground_state = ground_state[0, :]
    return np.ascontiguousarray(ground_state), float(values.reshape(-1)[0]), representatives


def save_ground_state(filename: str, ground_state, energy: float, representatives) -> None:
    """A file in the layout :func:`load_ground_state` (and the reference) reads."""
    content = {
        "hamiltonian": {"eigenvectors": np.asarray(ground_state, dtype=np.float64).reshape(1, -1),
                        "eigenvalues": np.asarray([energy], dtype=np.float64)},
        "basis": {"representatives": np.asarray(representatives, dtype=np.uint64)},
    }
    h5py = _h5py_or_none()
    if h5py is not None:
        with h5py.File(filename, "w") as out:
            for group, members in content.items():
                g = out.create_group(group)
                for key, value in members.items():
                    g[key] = value
        return
    from . import hdf5_lite

    hdf5_lite.write(filename, content)


def load_hamiltonian(filename: str):
    """The operator of a ``physical_systems/*.yaml`` file (common.py:783-788): plain bases and
    symmetry-adapted ones whose generators are in sector 0, with or without spin inversion (every
    shipped file); the result runs its action on the GPU.  Other sectors raise ``ValueError``."""
    import yaml

    from . import operators

    with open(filename, "r") as f:
        config = yaml.safe_load(f)
    return operators.Operator.from_config(config)


@dataclass
class SamplingResult:
    """common.py:264-267."""

    spins: np.ndarray
    weights: Optional[np.ndarray]


def monte_carlo_sampling(states, ground_state, number_samples: int,
                         sampled_power: float = 2) -> SamplingResult:
    """Seed states drawn with probability ~ |psi|^p from numpy's global legacy stream
    (common.py:270-279)."""
    p = np.abs(ground_state) ** sampled_power
    p /= np.sum(p)
    picks = np.random.choice(len(states), size=number_samples, replace=True, p=p)
    return SamplingResult(spins=np.asarray(states)[picks], weights=None)


def add_noise_to_amplitudes(ground_state, eps: float) -> np.ndarray:
    """psi -> sign(psi) |psi| exp(eps U(-1, 1)), renormalised (common.py:825-835)."""
    ground_state = np.asarray(ground_state, dtype=np.float64, order="C")
    assert ground_state.ndim == 1
    log_amplitude = np.log(np.abs(ground_state))
    noise = eps * 2 * (np.random.rand(log_amplitude.size) - 0.5)
    noisy = np.sign(ground_state) * np.exp(log_amplitude + noise)
    return noisy / np.linalg.norm(noisy)


def ground_state_to_log_coeff_fn(ground_state, basis):
    """Closure ``spins -> log|psi| + i pi [psi < 0]`` (common.py:806-822)."""
    ground_state = np.asarray(ground_state, dtype=np.float64, order="C")
    assert ground_state.ndim == 1
    with np.errstate(divide="ignore"):
        log_amplitude = np.log(np.abs(ground_state))
    phase = np.where(ground_state >= 0, 0, np.pi)

    def index_of(spins: np.ndarray) -> np.ndarray:
        spins = np.asarray(spins, dtype=np.uint64, order="C")
        if spins.ndim > 1:
            spins = spins[:, 0]
        return np.asarray(basis.batched_index(spins), dtype=np.int64)

    def at_index(where: np.ndarray) -> np.ndarray:
        return log_amplitude[where] + 1j * phase[where]

    def log_coeff_fn(spins: np.ndarray) -> np.ndarray:
        return at_index(index_of(spins))

    # the two halves of the closure, for callers that keep the positions (make_ising_model)
    log_coeff_fn.index_of = index_of
    log_coeff_fn.at_index = at_index
    return log_coeff_fn
