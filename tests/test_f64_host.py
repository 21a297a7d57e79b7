"""Float64 residual check, the part that needs no GPU: the two entry points are exported and declared, and the host-side builder of the
circulant derivative operators the kernel applies (reached through an undocumented test aid of the library) is the float64 spectral operator."""
import ctypes
import os
import re
from ctypes import POINTER, c_double, c_int, c_void_p

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_handle():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    return _lib, _lib.load()


def test_library_exports_the_float64_entry_points():
    _lib, lib = _lib_handle()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    for name, n_args in (("hn_laplacian_f64", 5), ("hn_residual_f64", 9)):
        m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
        assert m, f"{name} is not declared"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params) == n_args
        for p, a in zip(params, args):
            assert (a is c_int) == p.startswith("int "), (p, a)
            assert (a is c_void_p) == ("*" in p), (p, a)
        assert getattr(lib, name) is not None
    assert "hybridnet.py:540-556" in hdr and "spectral.py:31-79" in hdr
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # new entry points within ABI 7
    # without a context both calls fail cleanly
    assert lib.hn_laplacian_f64(None, None, None, 1, None) == -1
    assert lib.hn_residual_f64(None, None, None, None, 1, None, None, 1, None) == -1


def _operators(lib, n):
    fn = lib.hn_debug_f64_operators
    fn.restype = c_int
    fn.argtypes = [c_int, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    d1r, d1i, d2 = (np.empty((n, n), dtype=np.float64) for _ in range(3))
    assert fn(n, *(a.ctypes.data_as(POINTER(c_double)) for a in (d1r, d1i, d2))) == 0
    return d1r, d1i, d2


@pytest.mark.parametrize("n", [16, 48])
def test_host_operators_are_the_float64_spectral_derivatives(n):
    """D2 is real, circulant and symmetric.  D1 is circulant; its real part is antisymmetric, and its imaginary part is the Nyquist convention of the
    reference's k-grid and nothing else: the grid keeps k = -pi at index n/2 (spectral.py:126-127) instead of zeroing it, which contributes
    i k_nyq (-1)^(j-m) / n -- so D1 is NOT real for this grid, and the kernel carries that rank-one term.  Both agree with ifft(diag . fft(I))."""
    import oracle.helmnet_oracle as O
    _, lib = _lib_handle()
    d1r, d1i, d2 = _operators(lib, n)
    for d in (d1r, d1i, d2):                                   # circulant: D[j][m] = D[(j + 1) % n][(m + 1) % n]
        assert np.array_equal(d, np.roll(np.roll(d, 1, 0), 1, 1))
    k1 = O.k_grid_1d(n).astype(np.float32)                     # the reference's fp32 grid and its fp32 square, carried in float64
    k2 = -(k1 * k1)
    eye = np.eye(n)
    want1 = np.fft.ifft(1j * k1.astype(np.float64)[:, None] * np.fft.fft(eye, axis=0), axis=0)
    want2 = np.fft.ifft(k2.astype(np.float64)[:, None] * np.fft.fft(eye, axis=0), axis=0)
    assert np.abs(d1r + 1j * d1i - want1).max() <= 1e-13 * np.abs(want1).max()
    assert np.abs(d2 - want2).max() <= 1e-13 * np.abs(want2).max()
    assert np.abs(d2 - d2.T).max() <= 1e-13 * np.abs(d2).max()
    assert np.abs(d1r + d1r.T).max() <= 1e-13 * np.abs(d1r).max()
    sign = (-1.0) ** (np.arange(n)[:, None] - np.arange(n)[None, :])
    assert np.abs(d1i - float(k1[n // 2]) / n * sign).max() <= 1e-13 * np.abs(want1).max()
    assert np.abs(d1i).max() > 0.0


def test_host_operator_builder_rejects_illegal_sizes():
    _, lib = _lib_handle()
    fn = lib.hn_debug_f64_operators
    fn.restype = c_int
    fn.argtypes = [c_int, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    buf = (c_double * 1)()
    for n in (0, 8, 40, 4096):
        assert fn(n, buf, buf, buf) == -1
    assert fn(16, None, buf, buf) == -1
