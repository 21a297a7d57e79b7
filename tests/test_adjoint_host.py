"""Adjoint-state gradients, the part that needs no GPU: hn_fgmres_adjoint_cycle and hn_adjoint_grad are declared, exported and bound; the similarity
A^T ~ W A W^-1 that makes the adjoint system preconditionable by the learned network, with W restated here from the oracle's PML profile; the
gradient formula (sign, conjugation, the -2 omega^2 / sos^3 factor) against central differences of a dense float64 solve; and the host-side
refusals of solve_implicit / adjoint_solve / gmres_adjoint.  Every figure is printed before it is asserted (pytest -s)."""
import os
import re
from ctypes import c_double, c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PML, SIGMA_MAX, K, OMEGA = 8, 2.0, 1.0, 1.0


def _declared(hdr, name):
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_library_exports_the_adjoint_entry_points():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    for name, count in (("hn_fgmres_adjoint_cycle", 16), ("hn_adjoint_grad", 8)):
        params = _declared(hdr, name)
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params) == count, (name, len(args), len(params))
        for p, a in zip(params, args):
            want = c_void_p if "*" in p else c_double if p.startswith("double ") else c_float if p.startswith("float ") else c_int
            assert a is want, (name, p, a)
    # the argument list of the adjoint cycle is that of the forward flexible cycle
    assert [p.split()[-1] for p in _declared(hdr, "hn_fgmres_adjoint_cycle")] == [p.split()[-1] for p in _declared(hdr, "hn_fgmres_cycle")]
    assert _lib.SYMBOLS["hn_fgmres_adjoint_cycle"] == _lib.SYMBOLS["hn_fgmres_cycle"]
    grad = _declared(hdr, "hn_adjoint_grad")
    assert grad[1:7] == ["const float* lambda", "const float* u", "int src_batch", "int batch", "float* g_k_sq", "float* g_src"]
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # new entry points within ABI 7
    assert lib.hn_fgmres_adjoint_cycle(None, None, None, None, 1, 1, 1, 0.0, 1, 1.0, None, None, None, None, None, None) == -1
    assert lib.hn_adjoint_grad(None, None, None, 1, 1, None, None, None) == -1
    # no new profile kernel ids, and the older entry points are what they were
    src = open(os.path.join(REPO, "helmnet_amd", "csrc", "hn_internal.h")).read()
    assert re.search(r"KID_COUNT = 37\b", src)
    assert len(_lib.SYMBOLS["hn_fgmres_cycle"][1]) == 16 and len(_lib.SYMBOLS["hn_gmres_cycle"][1]) == 13


def _restated_weight(n):
    """W[i, j] = gamma_y[i] gamma_x[j], gamma = 1 + i sigma / k, from the oracle's own profile (not from the code under test)."""
    sigma, _, _ = O.pml_profiles(n, PML, SIGMA_MAX, K)
    gamma = 1.0 + 1j * sigma / K
    return gamma[:, None] * gamma[None, :]


@pytest.mark.parametrize("n", [32, 48])
def test_similarity_weight_makes_the_operator_nearly_complex_symmetric(n):
    from helmnet_amd.laplacian import adjoint_weight
    W = _restated_weight(n)
    got = adjoint_weight(n, PML, SIGMA_MAX, K)
    assert got.dtype == np.complex128 and got.shape == (n, n)
    err = float(np.abs(got - W).max())
    print(f"n={n}: max |adjoint_weight - restated W| = {err:.3e}, bar 1e-15")
    assert err <= 1e-15
    sos = 1.0 + 0.5 * np.random.default_rng(n).random((n, n))
    A = O.assemble_helmholtz_matrix((OMEGA / sos) ** 2, PML, SIGMA_MAX, K)
    w = W.reshape(-1)
    sim = (w[:, None] * A) / w[None, :]                        # W A W^-1
    rel = float(np.linalg.norm(A.T - sim) / np.linalg.norm(A))
    print(f"n={n}: |A^T - W A W^-1|_F / |A|_F = {rel:.3e}, bar 0.05 (twice the larger of 0.025 at 32 and 0.018 at 48)")
    assert rel <= 0.05


def _dense_problem(n, seed):
    rng = np.random.default_rng(seed)
    sos = 1.0 + 0.5 * rng.random((n, n))
    src = np.zeros((n, n), np.complex128)
    src[n // 2 - 2, n // 2] = 10.0
    src += 0.01 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    rx = n // 2 + 3
    d = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return sos, src, rx, d


def _loss(sos, src, rx, d):
    n = sos.shape[0]
    A = O.assemble_helmholtz_matrix((OMEGA / sos) ** 2, PML, SIGMA_MAX, K)
    u = np.linalg.solve(A, src.reshape(-1)).reshape(n, n)
    return 0.5 * float((np.abs(u[rx] - d) ** 2).sum()), u, A


def _planes(c):   # complex [n, n] -> float64 tensor [1, 2, n, n]
    return torch.from_numpy(np.stack([c.real, c.imag])[None])


def test_gradient_formula_against_central_differences_of_a_dense_float64_solve():
    """J = 1/2 sum |u[rx] - d|^2 with A u = src; lam = solve(A^H, dJ/du); the helper solve_implicit uses turns (lam, u, sos, omega) into dJ/dsos.
    <g, delta> against (J(+h delta) - J(-h delta)) / 2h, h = 1e-6, to 1e-6 relative -- for sos and for the source."""
    from helmnet_amd.autograd import adjoint_state_grads
    n, h = 32, 1e-6
    sos, src, rx, d = _dense_problem(n, 7)
    J, u, A = _loss(sos, src, rx, d)
    g = np.zeros((n, n), np.complex128)
    g[rx] = u[rx] - d                                           # dJ/du_re + i dJ/du_im
    lam = np.linalg.solve(A.conj().T, g.reshape(-1)).reshape(n, n)
    g_sos, g_k_sq = adjoint_state_grads(_planes(lam), _planes(u), torch.from_numpy(sos)[None, None], OMEGA)
    assert g_sos.dtype == torch.float64 and tuple(g_sos.shape) == (1, 1, n, n) and tuple(g_k_sq.shape) == (1, 1, n, n)
    want_k = -(np.conj(lam) * u).real
    assert float(np.abs(g_k_sq[0, 0].numpy() - want_k).max()) <= 1e-15 * float(np.abs(want_k).max())
    rng = np.random.default_rng(11)
    delta = rng.standard_normal((n, n))
    fd = (_loss(sos + h * delta, src, rx, d)[0] - _loss(sos - h * delta, src, rx, d)[0]) / (2 * h)
    an = float((g_sos[0, 0].numpy() * delta).sum())
    print(f"J = {J:.6e}; d/dsos: adjoint {an:.12e}  central difference {fd:.12e}  relative {abs(an - fd) / abs(fd):.3e}, bar 1e-6")
    assert abs(an - fd) <= 1e-6 * abs(fd)
    dsrc = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    fd = (_loss(sos, src + h * dsrc, rx, d)[0] - _loss(sos, src - h * dsrc, rx, d)[0]) / (2 * h)
    an = float((lam.real * dsrc.real + lam.imag * dsrc.imag).sum())          # g_src = lam, as two real planes
    print(f"d/dsrc: adjoint {an:.12e}  central difference {fd:.12e}  relative {abs(an - fd) / abs(fd):.3e}, bar 1e-6")
    assert abs(an - fd) <= 1e-6 * abs(fd)


def test_host_side_refusals():
    import inspect
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres_adjoint
    assert callable(Engine.fgmres_adjoint_cycle) and callable(Engine.adjoint_grad)
    p = inspect.signature(gmres_adjoint).parameters
    assert p["restart"].default == 20 and p["max_outer"].default == 50 and p["tol"].default == 1e-4 and p["precond_iterations"].default == 10
    assert p["precond_scale"].default is None and p["x0"].default is None
    p = inspect.signature(IterativeSolver.solve_implicit).parameters
    assert p["tol"].default == 1e-4 and p["adjoint_tol"].default is None and p["restart"].default == 20 and p["max_cycles"].default == 50
    assert p["precondition"].default == "learned" and p["precond_iterations"].default == 10 and p["x0"].default is None
    sos, g = torch.ones(1, 1, 16, 16), torch.zeros(1, 2, 16, 16)
    with pytest.raises(ValueError, match="precondition='learned' needs backend='hip'"):
        gmres_adjoint(None, sos, g, precondition="learned", backend="torch")
    with pytest.raises(ValueError, match="unknown precondition"):
        gmres_adjoint(None, sos, g, precondition="jacobi")
    with pytest.raises(ValueError, match="precond_iterations"):
        gmres_adjoint(None, sos, g, precondition="learned", precond_iterations=-1)
    s = IterativeSolver.from_exported_weights(); s.freeze()                  # on the CPU: nothing below may reach the library
    s.set_domain_size(32, source_location=[14, 16])
    with pytest.raises(ValueError, match="precondition='learned' needs backend='hip'"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 32), torch.ones(1, 1, 32, 32), precondition="learned", backend="torch")
    with pytest.raises(ValueError, match="right-hand side"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 16), torch.ones(1, 1, 32, 32))
    with pytest.raises(ValueError, match="right-hand side"):
        s.adjoint_solve(torch.zeros(3, 2, 32, 32), torch.ones(2, 1, 32, 32))
    with pytest.raises(ValueError, match="sos_maps"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 32), torch.ones(1, 32, 32))
    with pytest.raises(RuntimeError, match="grad"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 32), torch.ones(1, 1, 32, 32).requires_grad_(True))
    with pytest.raises(ValueError, match="sos must be"):
        s.solve_implicit(torch.ones(1, 1, 16, 16))
    with pytest.raises(ValueError, match="x0 must be"):
        s.solve_implicit(torch.ones(2, 1, 32, 32), x0=torch.zeros(1, 2, 32, 32))
    with pytest.raises(ValueError, match="unknown precondition"):
        s.solve_implicit(torch.ones(1, 1, 32, 32), precondition="ilu")
    s.set_domain_size((32, 48), source_location=[14, 16])
    for call in (lambda: s.solve_implicit(torch.ones(1, 1, 32, 48)), lambda: s.adjoint_solve(torch.zeros(1, 2, 32, 48), torch.ones(1, 1, 32, 48))):
        with pytest.raises(NotImplementedError, match=r"rectangular domain \(32 x 48\)"):
            call()
