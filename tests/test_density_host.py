"""Heterogeneous density, the part that needs no GPU: the three entry points declared, exported and bound; ``log_density_gradient`` against an analytic
gradient; the two float64 references of tests/density_common.py against each other (and density moving the solution); the refusals the front end
makes before any GPU work."""
import inspect
import math
import os
import re
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

import density_common as DC
import rect_common as R
from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(hdr, name):
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_the_binding_carries_the_three_entry_points():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    for name, sibling in (("hn_residual_medium", "hn_residual_lossy"), ("hn_step_medium", "hn_step_lossy"),
                          ("hn_fgmres_cycle_medium", "hn_fgmres_cycle_lossy")):
        params, old = _declared(hdr, name), _declared(hdr, sibling)
        # the lossy sibling's parameters with rho_grad directly behind k_sq_im
        at = old.index("const float* k_sq_im") + 1
        assert params == old[:at] + ["const float* rho_grad"] + old[at:], (name, params)
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = c_void_p if "*" in p else c_float if p.startswith("float ") else c_int
            assert a is want, (name, p, a)
        assert _lib.SYMBOLS[sibling][1] == args[:at] + args[at + 1:]
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # additions within ABI 7
    assert lib.hn_residual_medium(None, None, None, None, None, None, 1, None, 1, None) == -1
    assert lib.hn_step_medium(None, None, None, None, None, None, None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert lib.hn_fgmres_cycle_medium(None, None, None, None, None, None, 1, 1, 1, 0.0, 1, 1.0, None, None, None, None, None, None) == -1


def test_log_density_gradient_against_the_analytic_gradient():
    from helmnet_amd.density import log_density_gradient
    h, w, amp = 48, 80, 0.3
    x, y = torch.arange(w, dtype=torch.float64), torch.arange(h, dtype=torch.float64)
    for m in (1, 3, 7):
        # rho = exp(A cos(2 pi m x / W)): d ln rho / dx = -A (2 pi m / W) sin(2 pi m x / W), nothing along y -- and the same along y
        rx = torch.exp(amp * torch.cos(2 * math.pi * m * x / w)).view(1, 1, 1, w).expand(2, 1, h, w).contiguous()
        ry = torch.exp(amp * torch.cos(2 * math.pi * m * y / h)).view(1, 1, h, 1).expand(2, 1, h, w).contiguous()
        wx = (-amp * 2 * math.pi * m / w * torch.sin(2 * math.pi * m * x / w)).view(1, 1, w).expand(2, h, w)
        wy = (-amp * 2 * math.pi * m / h * torch.sin(2 * math.pi * m * y / h)).view(1, h, 1).expand(2, h, w)
        qx, qy = log_density_gradient(rx), log_density_gradient(ry)
        assert qx.dtype == torch.float64 and tuple(qx.shape) == (2, 2, h, w) and qx.is_contiguous()
        ex = max(float((qx[:, 0] - wx).abs().max()), float(qx[:, 1].abs().max()))
        ey = max(float((qy[:, 1] - wy).abs().max()), float(qy[:, 0].abs().max()))
        print(f"log_density_gradient {h}x{w} m={m}: max error along x {ex:.2e}, along y {ey:.2e}")
        assert ex <= 1e-12 and ey <= 1e-12
        # both at once, in fp32: the dtype of rho comes back, the planes are not swapped
        q32 = log_density_gradient((rx * ry).float())
        assert q32.dtype == torch.float32
        assert float((q32[:, 0].double() - wx).abs().max()) <= 1e-6 and float((q32[:, 1].double() - wy).abs().max()) <= 1e-6
    # only ratios matter: a constant map gives exact zeros, a constant factor nothing new to 1e-12
    assert not bool(log_density_gradient(torch.full((1, 1, h, w), 2.5, dtype=torch.float64)).any())
    assert not bool(log_density_gradient(torch.full((1, 1, h, w), 1700.0)).any())
    assert float((log_density_gradient(1000.0 * rx) - log_density_gradient(rx)).abs().max()) <= 1e-12
    # the Nyquist mode of a real field drops out
    alt = torch.exp(0.1 * torch.cos(math.pi * x)).view(1, 1, 1, w).expand(1, 1, h, w).contiguous()
    assert float(log_density_gradient(alt).abs().max()) <= 1e-12
    # the restatement the GPU tests use agrees with it
    sos, rho, q = DC.ring_medium(32)
    assert float((log_density_gradient(rho.double()).float() - q).abs().max()) <= 1e-7
    doc = log_density_gradient.__doc__
    assert "RATIOS" in doc and "smooth" in doc and "any gradient the caller prefers" in doc
    with pytest.raises(ValueError, match="positive"):
        log_density_gradient(torch.zeros(1, 1, h, w))


def test_the_two_references_agree_and_density_moves_the_solution():
    """n = 32, ring phantom, point source of amplitude 10 at [12, 16]: the float64 direct solution of the assembled A_rho has a residual of at most
    1e-11 * max|u| under the FFT composition (measured: 1e-14), and differs from the constant-density solution by 0.57 in max-norm (|u| about 4)."""
    n = 32
    sos, rho, q = DC.ring_medium(n)
    src = O.point_source_map(n, [12, 16], 10.0)
    t = R.tables(n, n)
    k_sq = ((1.0 / sos) ** 2).contiguous()
    assert 0.05 < float(q.abs().max()) < 0.6 and float(rho.max()) > 1.5
    for b in range(2):
        u, mat = DC.direct_solve(k_sq[b, 0].numpy(), None, q[b].numpy(), src.numpy()[0])
        ut = torch.from_numpy(u).unsqueeze(0)
        res = DC.residual(ut, k_sq[b:b + 1].double(), None, q[b:b + 1].double(), src.double(), t)
        scale = float(np.abs(u).max())
        u0 = O.direct_solve(sos[b, 0].numpy(), src.numpy()[0], *R.DOMAIN)
        moved = float(np.abs(u - u0).max())
        print(f"n={n} sample {b}: residual of the direct solution under the FFT composition {float(res.abs().max()):.2e} (max|u| {scale:.2f}); "
              f"density moves the solution by {moved:.3f}; cond {np.linalg.cond(mat):.0f}")
        assert float(res.abs().max()) <= 1e-11 * scale
        assert moved >= 0.1
    # with absorption too: the imaginary plane and the density term in one matrix
    k_im = (0.2 * (1.0 / sos) * 0.1).contiguous()
    u, _ = DC.direct_solve(k_sq[0, 0].numpy(), k_im[0, 0].numpy(), q[0].numpy(), src.numpy()[0])
    res = DC.residual(torch.from_numpy(u).unsqueeze(0), k_sq[:1].double(), k_im[:1].double(), q[:1].double(), src.double(), t)
    assert float(res.abs().max()) <= 1e-11 * float(np.abs(u).max())


def test_front_end_signatures_and_refusals_before_any_gpu_work():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres
    assert callable(Engine.residual_medium) and callable(Engine.step_medium) and callable(Engine.fgmres_cycle_medium)
    for f in (IterativeSolver.forward, IterativeSolver.n_steps, IterativeSolver.solve_to_tolerance, IterativeSolver.gmres, gmres):
        names = list(inspect.signature(f).parameters)
        assert names[-1] == "density" and inspect.signature(f).parameters["density"].default is None, f      # appended behind what was there
    assert inspect.signature(IterativeSolver.get_residual).parameters["rho_grad"].default is None
    sos = torch.ones(1, 1, 16, 16)
    rho = 1.0 + 0.1 * torch.rand(1, 1, 16, 16, generator=torch.Generator().manual_seed(1))
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.set_domain_size(16, source_location=[4, 8])
    with pytest.raises(ValueError, match="density needs backend='hip'"):
        gmres(s, sos, backend="torch", density=rho)
    with pytest.raises(NotImplementedError, match="refine=True"):
        gmres(s, sos, backend="hip", refine=True, density=rho)
    # a solver that is still on the CPU: the gradient refusal comes before the engine is asked for (which would raise its own RuntimeError)
    z = torch.zeros(1, 2, 16, 16)
    for call in (lambda: s.forward(sos.clone().requires_grad_(True), num_iterations=1, density=rho),
                 lambda: s.forward(sos, num_iterations=1, density=rho.clone().requires_grad_(True)),
                 lambda: s.forward(sos, num_iterations=1, absorption=torch.full_like(sos, 0.02).requires_grad_(True), density=rho),
                 lambda: s.solve_to_tolerance(sos.clone().requires_grad_(True), 1e-3, max_iterations=2, density=rho),
                 lambda: s.gmres(sos, density=rho.clone().requires_grad_(True)),
                 lambda: gmres(s, sos.clone().requires_grad_(True), backend="hip", density=rho),
                 lambda: s.n_steps(z.clone().requires_grad_(True), sos, z, 1, density=rho),
                 lambda: s.n_steps(z, sos, z, 1, absorption=0.02, density=rho.clone().requires_grad_(True)),
                 lambda: s.get_residual(z.clone().requires_grad_(True), sos, rho_grad=torch.zeros(1, 2, 16, 16))):
        with pytest.raises(RuntimeError, match="grad"):
            call()
    with pytest.raises(RuntimeError, match="with density runs without gradients"):
        s.forward(sos.clone().requires_grad_(True), num_iterations=1, density=rho)
    with pytest.raises(NotImplementedError, match="verify=True"):
        s.solve_to_tolerance(sos, 1e-3, max_iterations=2, verify=True, density=rho)
