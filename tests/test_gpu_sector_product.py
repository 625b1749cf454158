"""asp_sector_matvec (csrc/sector_basis.hip: k_sector_matvec) on ELL arrays of the test's own making
(tests/lanczos_cases.py): the product's law is exact — ``acc = diag[i] * x[i]``, then one fused
multiply-add per slot in slot order — so every named case must equal its restatement bit for bit, signed
zeros and subnormals included (tests/test_lanczos_cases.py shows which case tells which wrong reading of
the law apart).  Around the call: y's neighbours and the inputs stay untouched, the degenerate calls
(width 0, n = 0, null arguments, x aliasing y) do what include/asp.h says."""
import ctypes

import numpy as np
import pytest

import lanczos_cases
from lanczos_cases import PRODUCT_CASES

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300


class _Ell:
    """What sector_ed.SectorMatrix.matvec reads of its object: n, width, idx, val and diag on the device."""

    def __init__(self, idx, val, diag):
        import torch

        self.width, self.n = idx.shape
        self.idx = torch.tensor(idx.view(np.int32), device="cuda")  # (the device array holds the u32 as i32)
        self.val = torch.tensor(val, device="cuda")
        self.diag = torch.tensor(diag, device="cuda")

    def matvec(self, x, out=None):
        from annealing_sign_problem_amd import sector_ed

        return sector_ed.SectorMatrix.matvec(self, x, out=out)


def _same_bits(tensor, array):
    host = tensor.cpu().numpy()
    return host.shape == array.shape and host.tobytes() == array.tobytes()


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


@pytest.mark.parametrize("name", list(PRODUCT_CASES))
def test_product_equals_the_law_bit_for_bit(name):
    import torch

    idx, val, diag, x = PRODUCT_CASES[name]
    want = lanczos_cases.product_law(name)
    matrix = _Ell(idx, val, diag)
    n = matrix.n
    device_x = torch.tensor(x, device="cuda")
    guarded = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    y = guarded[1: n + 1]
    assert y.is_contiguous() and y.data_ptr() == guarded.data_ptr() + 8
    assert matrix.matvec(device_x, out=y) is y
    got = guarded.cpu().numpy()
    assert got[0] == SENTINEL and got[-1] == SENTINEL             # one element on each side of y
    assert got[1:-1].tobytes() == want.tobytes(), np.flatnonzero(got[1:-1].view(np.uint64) != want.view(np.uint64))[:8]
    assert not np.any(got[1:-1] == SENTINEL)
    # the inputs are only read
    assert _same_bits(matrix.idx, idx.view(np.int32)) and _same_bits(matrix.val, val)
    assert _same_bits(matrix.diag, diag) and _same_bits(device_x, x)
    # and a product into fresh memory gives the same bytes
    assert _same_bits(matrix.matvec(device_x), want)


def test_width_zero_takes_null_arrays_and_n_zero_writes_nothing():
    import torch

    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    for n in (1, 65, 257):
        idx, val, diag, x = PRODUCT_CASES["n%d_w0" % n]
        assert idx.shape == (0, n)
        device_diag, device_x = torch.tensor(diag, device="cuda"), torch.tensor(x, device="cuda")
        guarded = torch.full((n + 2,), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.asp_sector_matvec(n, 0, None, None, _ptr(device_diag), _ptr(device_x), _ptr(guarded[1:])))
        got = guarded.cpu().numpy()
        assert got[0] == SENTINEL and got[-1] == SENTINEL
        assert got[1:-1].tobytes() == (diag * x).tobytes() == lanczos_cases.product_law("n%d_w0" % n).tobytes()
    # n = 0: returns 0 whatever the other arguments are, and writes nothing
    idx, val, diag, x = PRODUCT_CASES["n65_w7"]
    matrix, device_x = _Ell(idx, val, diag), torch.tensor(x, device="cuda")
    y = torch.full((65,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert lib.asp_sector_matvec(0, 7, _ptr(matrix.idx), _ptr(matrix.val), _ptr(matrix.diag), _ptr(device_x), _ptr(y)) == 0
    assert lib.asp_sector_matvec(0, 0, None, None, None, None, None) == 0
    assert lib.asp_sector_matvec(0, 7, None, None, None, None, _ptr(y)) == 0
    torch.cuda.synchronize()
    assert np.all(y.cpu().numpy() == SENTINEL)


def test_refused_calls_write_nothing_and_the_next_product_is_the_same():
    import torch

    from annealing_sign_problem_amd import _lib

    lib = _lib.load()
    idx, val, diag, x = PRODUCT_CASES["n257_w7"]
    want = lanczos_cases.product_law("n257_w7")
    matrix, device_x = _Ell(idx, val, diag), torch.tensor(x, device="cuda")
    n, width = matrix.n, matrix.width
    first = matrix.matvec(device_x)
    assert _same_bits(first, want)
    y = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    i, v, d, xs, out = _ptr(matrix.idx), _ptr(matrix.val), _ptr(matrix.diag), _ptr(device_x), _ptr(y)
    refused = [((n, width, i, v, None, xs, out), "null argument"),
               ((n, width, i, v, d, None, out), "null argument"),
               ((n, width, i, v, d, xs, None), "null argument"),
               ((n, width, None, v, d, xs, out), "null argument"),
               ((n, width, i, None, d, xs, out), "null argument"),
               ((n, width, i, v, d, out, out), "x and y must not alias"),
               ((n, 0, None, None, d, out, out), "x and y must not alias")]
    for arguments, message in refused:
        assert lib.asp_sector_matvec(*arguments) == -3, message  # ASP_ERR_INVALID
        assert _lib.last_error() == message
        with pytest.raises(_lib.AspError) as err:
            _lib.check(lib.asp_sector_matvec(*arguments))
        assert err.value.code == -3 and message in str(err.value)
        torch.cuda.synchronize()
        assert np.all(y.cpu().numpy() == SENTINEL)
        assert _same_bits(matrix.idx, idx.view(np.int32)) and _same_bits(matrix.val, val)
        assert _same_bits(matrix.diag, diag) and _same_bits(device_x, x)
        # the same arrays again after the refusal: the same bytes, and the error is cleared
        again = matrix.matvec(device_x)
        assert _same_bits(again, want) and _lib.last_error() == ""
    # SectorMatrix.matvec's own checks
    for bad in (device_x.to(torch.float32), device_x[:-1], torch.tensor(np.repeat(x, 2), device="cuda")[::2]):
        with pytest.raises(ValueError):
            matrix.matvec(bad)
    with pytest.raises(_lib.AspError):
        matrix.matvec(device_x, out=device_x)
    assert _same_bits(device_x, x) and _same_bits(matrix.matvec(device_x), want)
