"""Heterogeneous density: the gradient of ln rho the variable-density operator takes (extension; the reference's Python side has a constant
density, its MATLAB side sets ``medium.density`` in matlab/skull_example.m and builds it in matlab/skull2medium.m).

With the PML stretch ``gamma = 1 + i sigma / k`` the solver's Laplacian is, per axis, ``a du + b d2u`` (laplacian.py).  A density that varies turns
``(1/gamma) d((1/gamma) du)`` into ``rho (1/gamma) d((1/rho)(1/gamma) du) = a du + b d2u - b q du`` with ``q = d ln rho``, so

    A_rho u = L(u) - b_x q_x d_x u - b_y q_y d_y u + (k_sq + i k_sq_im) u

(``hn_residual_medium``, ``hn_step_medium``, ``hn_fgmres_cycle_medium``; its adjoint and the adjoint-state gradients of a converged solve:
``hn_residual_vjp_medium``, ``hn_fgmres_adjoint_cycle_medium``, ``hn_adjoint_grad_medium``, which returns dJ/dq -- ``log_density_gradient_vjp``
below turns that into dJ/drho).  This is the expanded form, not the conservative discretisation of
``rho div((1/rho) grad u)``: on a grid the two differ by 1-2 % for a smooth ``u`` and by O(1) for white noise, because products alias.
"""
from __future__ import annotations

import numpy as np
import torch

from .laplacian import k_grid


def log_density_gradient(rho: torch.Tensor) -> torch.Tensor:
    """``rho`` [B,1,H,W] (positive) -> [B,2,H,W]: plane 0 is d ln rho / dx along the LAST index (length W, the axis of ``sigma_x``), plane 1 is
    d ln rho / dy along the first spatial index (length H), per grid point -- the ``rho_grad`` of ``Engine.residual_medium``.

    The real part of the Fourier derivative of ln rho on the solver's k grid (laplacian.k_grid), computed in float64 on the tensor's device and
    returned in the dtype of ``rho``; the Nyquist mode of a real field has a purely imaginary derivative and so drops out.

    Only RATIOS of rho matter: a constant factor leaves ln rho's gradient alone (and a constant rho gives exact zeros).  A jump in rho makes the
    spectral derivative ring (Gibbs); smooth the map first, as k-Wave users do.  The C entry points take any gradient the caller prefers -- finite
    differences of a smoothed map, an analytic one -- this function is a convenience, not part of the operator's definition."""
    if not isinstance(rho, torch.Tensor) or rho.dim() != 4 or rho.shape[1] != 1:
        raise ValueError(f"rho: expected a [B, 1, H, W] tensor, got {tuple(getattr(rho, 'shape', ()))}")
    if not rho.is_floating_point():
        raise TypeError("rho must be a floating-point tensor")
    if not bool((rho > 0).all()):
        raise ValueError("rho must be positive everywhere")
    h, w = int(rho.shape[2]), int(rho.shape[3])
    ln = rho.detach().to(torch.float64).log()
    ln = ln - ln[:, :, :1, :1]   # ln(rho / rho[0, 0]): the same gradient, and a constant map is exact zeros whatever the transform's radix
    kx = torch.from_numpy(np.ascontiguousarray(k_grid(w))).to(ln.device).view(1, 1, 1, w)
    ky = torch.from_numpy(np.ascontiguousarray(k_grid(h))).to(ln.device).view(1, 1, h, 1)
    qx = torch.fft.ifft(1j * kx * torch.fft.fft(ln, dim=3), dim=3).real
    qy = torch.fft.ifft(1j * ky * torch.fft.fft(ln, dim=2), dim=2).real
    return torch.cat([qx, qy], 1).to(rho.dtype).contiguous()


def log_density_gradient_vjp(g_rho_grad: torch.Tensor, rho: torch.Tensor) -> torch.Tensor:
    """dJ/drho [B,1,H,W] from ``g_rho_grad`` = dJ/dq [B,2,H,W] (``Engine.adjoint_grad_medium``), q = ``log_density_gradient(rho)``.

    With G the map of ``log_density_gradient`` along one axis (real and antisymmetric: its transpose is -G, the Nyquist mode drops out both ways),
    dJ/dln rho = -(G_x dJ/dq_x + G_y dJ/dq_y) and dJ/drho = dJ/dln rho / rho.  Computed in float64 on the tensor's device and returned in the dtype of
    ``rho``.  ``rho`` may have been broadcast along the batch ([1,1,H,W]): the result then has the batch of ``g_rho_grad`` and the caller sums."""
    if not isinstance(rho, torch.Tensor) or rho.dim() != 4 or rho.shape[1] != 1:
        raise ValueError(f"rho: expected a [B, 1, H, W] tensor, got {tuple(getattr(rho, 'shape', ()))}")
    if not isinstance(g_rho_grad, torch.Tensor) or g_rho_grad.dim() != 4 or g_rho_grad.shape[1] != 2 or g_rho_grad.shape[2:] != rho.shape[2:] \
            or rho.shape[0] not in (1, g_rho_grad.shape[0]):
        raise ValueError(f"g_rho_grad: expected a [B, 2, H, W] tensor on the grid of rho {tuple(rho.shape)}, got {tuple(getattr(g_rho_grad, 'shape', ()))}")
    if not rho.is_floating_point():
        raise TypeError("rho must be a floating-point tensor")
    if not bool((rho > 0).all()):
        raise ValueError("rho must be positive everywhere")
    h, w = int(rho.shape[2]), int(rho.shape[3])
    g = g_rho_grad.detach().to(device=rho.device, dtype=torch.float64)
    kx = torch.from_numpy(np.ascontiguousarray(k_grid(w))).to(g.device).view(1, 1, 1, w)
    ky = torch.from_numpy(np.ascontiguousarray(k_grid(h))).to(g.device).view(1, 1, h, 1)
    gx = torch.fft.ifft(1j * kx * torch.fft.fft(g[:, 0:1], dim=3), dim=3).real
    gy = torch.fft.ifft(1j * ky * torch.fft.fft(g[:, 1:2], dim=2), dim=2).real
    return (-(gx + gy) / rho.detach().to(torch.float64)).to(rho.dtype).contiguous()
