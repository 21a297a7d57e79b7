"""GMRES to float64 accuracy, the part that needs no GPU: hn_gmres_refine_cycle is declared, exported and bound; the host loop of the refinement is
exercised with a scripted cycle; and the METHOD -- float64 residual, fp32 GMRES(m) on the scaled correction equation, float64 update -- is modelled
in numpy on a small dense matrix.  That model is the specification the device code is compared with (tests/test_gmres_refine_gpu.py)."""
import os
import re
from ctypes import c_double, c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- header, binding, symbol
def test_library_exports_hn_gmres_refine_cycle():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    m = re.search(r"int hn_gmres_refine_cycle\((.*?)\);", hdr, re.S)
    assert m, "hn_gmres_refine_cycle is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, args = _lib.SYMBOLS["hn_gmres_refine_cycle"]
    assert res is c_int and len(args) == len(params) == 15
    for p, a in zip(params, args):
        want = c_void_p if "*" in p else c_double if p.startswith("double ") else c_float if p.startswith("float ") else c_int
        assert a is want, (p, a)
    assert params[1] == "double* x" and params[7] == "double tol" and params[8] == "float inner_floor" and params[13] == "double* rmse64"
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # a new entry point within ABI 7
    assert lib.hn_gmres_refine_cycle(None, None, None, None, 1, 1, 1, 0.0, 0.0, None, None, None, None, None, None) == -1
    # the old entry point is still what it was
    assert _lib.SYMBOLS["hn_gmres_cycle"][1][7] is c_float and len(_lib.SYMBOLS["hn_gmres_cycle"][1]) == 13


def test_public_methods_exist_and_refuse_before_any_gpu_work():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres
    assert callable(Engine.gmres_refine_cycle) and callable(IterativeSolver.gmres64) and callable(IterativeSolver.reference_error)
    sos = torch.ones(1, 1, 16, 16)
    with pytest.raises(ValueError, match="refine"):
        gmres(None, sos, backend="torch", refine=True)
    with pytest.raises(RuntimeError, match="grad"):
        gmres(None, sos.clone().requires_grad_(True), backend="hip", refine=True)
    with pytest.raises(RuntimeError, match="grad"):
        gmres(None, sos, x0=torch.zeros(1, 2, 16, 16, requires_grad=True), backend="hip", refine=True)


# ---------------------------------------------------------------------------------------------- the driver
class _Script:
    """A scripted refinement: per call (rmse64 [B], table [m + 1, B], k_used [B])."""

    def __init__(self, cycles):
        self.cycles, self.calls = list(cycles), 0

    def cycle(self):
        out = self.cycles[self.calls]
        self.calls += 1
        return np.asarray(out[0], np.float64), np.asarray(out[1], np.float32), np.asarray(out[2])


def test_driver_stops_on_the_first_cycle_that_finds_every_sample_below_tol():
    from helmnet_amd.gmres import drive_refinement
    tol = 1e-9
    t1 = [[1.0, 1.0], [0.1, 0.2], [1e-3, 0.05]]
    t2 = [[1.0, 1.0], [1e-4, 0.3], [1e-4, 0.01]]       # sample 0 stops after one inner step, its later rows repeat
    t3 = [[1.0, 1.0], [1.0, 0.1], [1.0, 1e-3]]         # sample 0 is below tol in float64: k_used 0, rows repeat row 0
    t4 = [[1.0, 1.0]] * 3                              # the final check: nothing runs
    s = _Script([([3e-2, 2e-2], t1, [2, 2]), ([4e-5, 1e-3], t2, [1, 2]), ([5e-10, 2e-5], t3, [0, 2]), ([5e-10, 3e-10], t4, [0, 0]),
                 ([0.0, 0.0], t4, [0, 0])])
    out = drive_refinement(s.cycle, max_cycles=10, tol=tol)
    assert out["converged"] and out["cycles"] == 4 and s.calls == 4            # the fifth scripted cycle is never asked for
    h = np.stack(out["history"])
    assert h.dtype == np.float64 and h.shape == (4, 2)
    assert np.array_equal(h, np.array([[3e-2, 2e-2], [4e-5, 1e-3], [5e-10, 2e-5], [5e-10, 3e-10]]))   # float64 values, unrounded
    assert out["iterations_per_sample"].dtype == np.int64 and out["iterations_per_sample"].tolist() == [3, 6]
    assert out["iterations"] == 6                                              # lock step: 2 + 2 + 2 + 0
    assert len(out["tables"]) == 4 and out["tables"][1].dtype == np.float32 and np.array_equal(out["tables"][1], np.asarray(t2, np.float32))


def test_driver_start_below_tol_is_one_call_and_no_iteration():
    from helmnet_amd.gmres import drive_refinement
    s = _Script([([1e-12, 0.0], [[1.0, 0.0], [1.0, 0.0]], [0, 0])])
    out = drive_refinement(s.cycle, max_cycles=5, tol=1e-10)
    assert out["converged"] and out["cycles"] == 1 and out["iterations"] == 0 and out["iterations_per_sample"].tolist() == [0, 0]
    assert len(out["history"]) == 1


def test_driver_not_converged_when_max_cycles_runs_out():
    from helmnet_amd.gmres import drive_refinement
    t = [[1.0], [0.5], [0.25]]
    s = _Script([([1.0 / 4 ** i], t, [2]) for i in range(6)])
    out = drive_refinement(s.cycle, max_cycles=3, tol=1e-10)
    assert not out["converged"] and out["cycles"] == 3 and s.calls == 3
    assert out["iterations"] == 6 and out["iterations_per_sample"].tolist() == [6]
    assert np.array_equal(np.stack(out["history"])[:, 0], np.array([1.0, 0.25, 0.0625]))
    # a NaN residual never counts as below the tolerance
    s = _Script([([float("nan")], t, [2])] * 2)
    out = drive_refinement(s.cycle, max_cycles=2, tol=1e-10)
    assert not out["converged"] and out["cycles"] == 2
    out = drive_refinement(s.cycle, max_cycles=0, tol=1e-10)
    assert not out["converged"] and out["cycles"] == 0 and out["history"] == [] and out["iterations"] == 0


# ---------------------------------------------------------------------------------------------- the method, in numpy
def _gmres_cycle(A, b, x, m, tol, dtype):
    """One cycle of GMRES(m) on A x = b from x, every vector and the Hessenberg matrix in ``dtype`` (complex64: the device's fp32 cycle; the small
    least-squares problem in complex128 on that matrix, as the device's Givens rotations are).  Stops at the first inner step whose estimate of
    |r| is below tol.  Returns the new x."""
    real = np.float32 if dtype == np.complex64 else np.float64
    A, b, x = A.astype(dtype), b.astype(dtype), x.astype(dtype)
    r = b - A @ x
    beta = real(np.linalg.norm(r))
    if beta < tol or beta == 0:
        return x
    Q = np.zeros((m + 1, b.size), dtype)
    H = np.zeros((m + 1, m), dtype)
    Q[0] = r / beta
    k_used = m
    for k in range(m):
        w = A @ Q[k]
        for _ in range(2):                                # two passes of classical Gram-Schmidt
            h = (Q[: k + 1].conj() @ w).astype(dtype)
            w = (w - h @ Q[: k + 1]).astype(dtype)
            H[: k + 1, k] += h
        hn = real(np.linalg.norm(w))
        H[k + 1, k] = hn
        Q[k + 1] = w / max(hn, real(1e-30))
        e1 = np.zeros(k + 2, np.complex128); e1[0] = beta
        Hk = H[: k + 2, : k + 1].astype(np.complex128)
        y = np.linalg.lstsq(Hk, e1, rcond=None)[0]
        if np.linalg.norm(e1 - Hk @ y) < tol:
            k_used = k + 1
            break
    e1 = np.zeros(k_used + 1, np.complex128); e1[0] = beta
    y = np.linalg.lstsq(H[: k_used + 1, :k_used].astype(np.complex128), e1, rcond=None)[0].astype(dtype)
    return (x + y @ Q[:k_used]).astype(dtype)


def test_numpy_model_refinement_reaches_float64_accuracy_where_fp32_gmres_stalls():
    """Float64 residual + fp32 GMRES(m) on A d = r / s from d = 0 + float64 update: the true residual falls below 1e-10 of its start.  The same number
    of cycles of GMRES(m) with a fp32 iterate and a fp32 residual stalls at fp32's floor."""
    rng = np.random.default_rng(7)
    N, m, cycles = 96, 10, 12
    A = (2.0 + 0.5j) * np.eye(N) + 0.9 * (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) / np.sqrt(2 * N)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    rms = lambda r: float(np.sqrt((np.abs(r) ** 2).sum() / (2 * N)))  # noqa: E731
    start = rms(b)
    # refinement
    x, trace = np.zeros(N, np.complex128), []
    for _ in range(cycles):
        r = b - A @ x                                      # float64
        s = max(rms(r), 1e-300)
        trace.append(s / start)
        d = _gmres_cycle(A, (r / s).astype(np.complex64), np.zeros(N, np.complex64), m, 1e-6 * np.sqrt(2 * N), np.complex64)   # fp32, from d = 0
        assert d.dtype == np.complex64
        x = x + s * d.astype(np.complex128)                # float64
    refined = rms(b - A @ x) / start
    # plain fp32 restarted GMRES: fp32 iterate, fp32 residual
    x32 = np.zeros(N, np.complex64)
    for _ in range(cycles):
        x32 = _gmres_cycle(A, b, x32, m, 0.0, np.complex64)
    assert x32.dtype == np.complex64
    plain = rms(b - A @ x32.astype(np.complex128)) / start
    print(f"true residual / start after {cycles} cycles of GMRES({m}): refined {refined:.3e}, plain fp32 {plain:.3e}")
    print("refinement trace:", " ".join(f"{t:.1e}" for t in trace))
    assert refined < 1e-10, refined
    assert plain > 1e-8, plain                             # fp32's floor: about 1e-7 of the right-hand side, three decades above the refined run
    assert plain > 100 * refined
    # a residual of exactly zero: s is the clamp, the scaled right-hand side is zero, nothing divides by zero, x stays
    x0 = np.zeros(N, np.complex128)
    r = np.zeros(N, np.complex128)
    s = max(rms(r), 1e-300)
    d = _gmres_cycle(A, (r / s).astype(np.complex64), np.zeros(N, np.complex64), m, 1e-6, np.complex64)
    assert not np.isnan(d).any() and np.array_equal(x0 + s * d.astype(np.complex128), x0)
