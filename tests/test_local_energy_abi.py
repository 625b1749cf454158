"""The C ABI of the local energies (asp_operator_local_energy, include/asp.h) without a device: the
symbol, the header against the bindings, every validation branch — all of which run before any device work and
before any output is written, with the offending index in the message —, the calls that need no device, and the
Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, TOO_LARGE = -3, None  # (TOO_LARGE is read from the header below)
SENTINEL = 12345.5
FAKE = ctypes.c_void_p(0x1000)  # an operator that does not exist: never dereferenced, a check fails first


def _u64(values):
    return np.array(values, dtype=np.uint64)


class _Outputs:
    def __init__(self, n):
        self.hphi = np.full(max(n, 1), SENTINEL)
        self.eloc = np.full(max(n, 1), SENTINEL)
        self.missing = np.full(max(n, 1), 77, dtype=np.uint32)

    def untouched(self):
        return bool(np.all(self.hphi == SENTINEL) and np.all(self.eloc == SENTINEL) and np.all(self.missing == 77))


def _call(op, offsets, keys, phi, rows, out, segments=None, n=None, eloc=True):
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    segments = (0 if offsets is None else offsets.size - 1) if segments is None else segments
    n = (0 if rows is None else rows.size) if n is None else n
    return lib.asp_operator_local_energy(op, segments, _lib.ptr(offsets), _lib.ptr(keys), _lib.ptr(phi), n,
                                         _lib.ptr(rows), _lib.ptr(out.hphi) if out else None,
                                         _lib.ptr(out.eloc) if out and eloc else None,
                                         _lib.ptr(out.missing) if out else None)


def _header():
    with open(os.path.join(ROOT, "include", "asp.h")) as f:
        return f.read()


def test_library_exports_and_header_declares_the_symbol():
    from annealing_sign_problem_amd import _lib, build

    lib = _lib.load()
    raw = ctypes.CDLL(_lib.library_path())
    assert "asp_operator_local_energy" in _lib.SIGNATURES and hasattr(lib, "asp_operator_local_energy")
    assert raw.asp_operator_local_energy is not None
    text = _header()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert ("int asp_operator_local_energy(asp_operator const *op, uint64_t num_segments, uint64_t const *offsets, "
            "uint64_t const *keys, double const *phi, uint64_t num_rows, uint64_t const *rows, double *hphi, "
            "double *eloc, uint32_t *missing);") in header
    p, u64 = ctypes.c_void_p, ctypes.c_uint64
    assert _lib.SIGNATURES["asp_operator_local_energy"] == (ctypes.c_int, [p, u64, p, p, p, u64, p, p, p, p])
    assert "ASP-ELOC-1" in text
    assert "operator_local_energy.hip" in build.SOURCES


def test_every_validation_branch_runs_before_any_device_work_and_before_any_output():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    offsets = _u64([0, 3, 3, 5])
    keys = _u64([3, 5, 6, 5, 9])
    phi = np.array([0.6, -0.8, 0.25, 1.5, -2.0])
    rows = _u64([4, 0, 0, 3])
    out = _Outputs(4)

    def refused(message, *args, **keywords):
        assert _call(*args, **keywords) == INVALID, message
        assert message in _lib.last_error(), _lib.last_error()
        assert out.untouched()

    refused("null operator", None, offsets, keys, phi, rows, out)
    refused("null offsets with 3 segments", FAKE, None, keys, phi, rows, out, segments=3)
    refused("offsets[0] is not 0", FAKE, _u64([1, 3, 3, 5]), keys, phi, rows, out)
    refused("offsets decrease at index 2", FAKE, _u64([0, 3, 2, 5]), keys, phi, rows, out)
    refused("offsets decrease at index 3", FAKE, _u64([0, 3, 3, 2]), keys, phi, rows, out)
    refused("null keys or phi with 5 table entries", FAKE, offsets, None, phi, rows, out)
    refused("null keys or phi with 5 table entries", FAKE, offsets, keys, None, rows, out)
    refused("the keys of segment 0 are not sorted and unique", FAKE, offsets, _u64([3, 6, 5, 5, 9]), phi, rows, out)
    refused("the keys of segment 0 are not sorted and unique", FAKE, offsets, _u64([3, 3, 6, 5, 9]), phi, rows, out)
    refused("the keys of segment 2 are not sorted and unique", FAKE, offsets, _u64([3, 5, 6, 9, 5]), phi, rows, out)
    refused("null rows with 4 rows", FAKE, offsets, keys, phi, None, out, n=4)
    refused("row 2 points at entry 5 of a table of 5", FAKE, offsets, keys, phi, _u64([4, 0, 5, 3]), out)
    refused("row 0 points at entry 0 of a table of 0", FAKE, None, None, None, _u64([0]), out)
    for bad in (0.0, -0.0, np.nan, np.inf, -np.inf):
        wrong = phi.copy()
        wrong[3] = bad
        refused("row 3 has a zero, NaN or infinite amplitude", FAKE, offsets, keys, wrong, rows, out)
    # (a key that repeats in ANOTHER segment is legal — entries 1 and 3 hold state 5 — and an amplitude of zero
    # away from the rows, or with eloc NULL, is too: tests/test_gpu_local_energy.py)
    assert _lib.gpu_touched() == touched


def test_sizes_beyond_the_index_range_are_refused():
    from annealing_sign_problem_amd import _lib

    _lib.load()
    touched = _lib.gpu_touched()
    code = int(re.search(r"ASP_ERR_TOO_LARGE\s*=\s*(-?\d+)", _header()).group(1))
    out = _Outputs(1)
    keys, phi, rows = _u64([3]), np.array([1.0]), _u64([0])
    # T = 2^32 - 1 (only the offsets say so: nothing of that length is read before the size check)
    assert _call(FAKE, _u64([0, 2 ** 32 - 1]), keys, phi, rows, out) == code
    assert "2^32" in _lib.last_error() and out.untouched()
    assert _call(FAKE, _u64([0, 1]), keys, phi, rows, out, n=2 ** 31 - 1) == code
    assert "2^31" in _lib.last_error() and out.untouched()
    assert _lib.gpu_touched() == touched


def test_no_rows_need_no_device():
    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    touched = _lib.gpu_touched()
    out = _Outputs(0)
    offsets, keys, phi = _u64([0, 2, 2]), _u64([3, 5]), np.array([0.0, np.nan])
    assert _call(FAKE, offsets, keys, phi, None, out) == 0 and lib.asp_last_error_code() == 0
    assert _call(FAKE, offsets, keys, phi, None, None) == 0
    assert _call(FAKE, None, None, None, None, None) == 0     # no segments, no table, no rows
    assert _call(FAKE, _u64([0]), None, None, None, out) == 0  # offsets of zero segments
    assert _call(None, None, None, None, None, None) == INVALID
    # the table is still checked
    assert _call(FAKE, offsets, keys[::-1].copy(), phi, None, out) == INVALID
    assert out.untouched() and _lib.gpu_touched() == touched


class _Foreign:
    """An operator object that is not this package's: only its own batched_apply."""

    class basis:
        number_spins = 4

    def batched_apply(self, spins):
        raise AssertionError("not reached")


def test_python_surface():
    from annealing_sign_problem_amd import _lib, common, local_energy, operators

    touched = _lib.gpu_touched()
    parameters = inspect.signature(operators.DeviceOperator.local_energy).parameters
    assert list(parameters) == ["self", "keys", "phi", "offsets", "rows"]
    assert parameters["offsets"].default is None and parameters["rows"].default is None
    assert list(inspect.signature(common.local_energies).parameters) == ["hamiltonian", "spins", "signed_psi", "rows"]
    assert inspect.signature(common.local_energies).parameters["rows"].default is None
    assert list(inspect.signature(common.variational_energy).parameters) == ["hamiltonian", "spins", "signed_psi"]
    assert "local_energies" in common.__all__ and "variational_energy" in common.__all__
    spins = np.array([3, 5, 6], dtype=np.uint64)
    with pytest.raises(NotImplementedError, match="foreign"):
        common.local_energies(_Foreign(), spins, np.ones(3))
    with pytest.raises(NotImplementedError, match="foreign"):
        common.variational_energy(_Foreign(), spins, np.ones(3))
    with pytest.raises(NotImplementedError, match="foreign"):
        local_energy.sample_local_energies(_Foreign(), np.ones(3), spins, lambda s: np.zeros(len(s)), 1, 1e-6)
    sample = inspect.signature(local_energy.sample_local_energies).parameters
    assert list(sample)[:10] == ["hamiltonian", "ground_state", "samples", "log_psi_fn", "order", "global_cutoff",
                                 "signs", "external_field", "seed", "jobs"]
    assert sample["signs"].default == "greedy" and sample["external_field"].default is False
    assert sample["jobs"].default == 1
    with pytest.raises(ValueError, match="invalid signs"):
        local_energy.sample_local_energies(_Foreign(), np.ones(3), spins, None, 1, 1e-6, signs="best")
    assert _lib.gpu_touched() == touched


def test_command_line_and_summary():
    from annealing_sign_problem_amd import local_energy

    args = local_energy.parse_command_line(["--model", "heisenberg_kagome_16", "--output", "x.csv"])
    assert (args.signs, args.order, args.external_field, args.noise, args.jobs, args.hdf5) == (
        "greedy", 2, False, 0, 1, None)
    assert args.number_samples == 1000 and args.sampled_power == 2.0
    args = local_energy.parse_command_line(
        ["--model", "heisenberg_kagome_18", "--hdf5", "g.h5", "--number-samples", "10", "--sampled-power", "1.5",
         "--order", "1", "--global-cutoff", "1e-4", "--signs", "exact", "--noise", "0.1", "--external-field",
         "--seed", "7", "--jobs", "3", "--output", "y.csv"])
    assert (args.signs, args.order, args.external_field, args.noise, args.jobs, args.seed) == (
        "exact", 1, True, 0.1, 3, 7)
    with pytest.raises(SystemExit):
        local_energy.parse_command_line(["--model", "m", "--output", "x.csv", "--signs", "best"])
    # (state, size, E_loc, missing, count): the mean is weighted by the counts
    results = [(3, 25, -1.0, 0, 3), (5, 25, 3.0, 0, 1)]
    mean, error = local_energy.weighted_mean(results)
    assert mean == 0.0
    samples = np.array([-1.0, -1.0, -1.0, 3.0])
    assert error == pytest.approx(samples.std(ddof=1) / 2.0, rel=1e-15)
    assert np.isnan(local_energy.weighted_mean([(3, 25, -1.0, 0, 1)])[1])
