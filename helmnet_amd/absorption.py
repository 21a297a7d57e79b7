"""Absorbing media: the complex squared wavenumber of a medium with loss (extension; the reference's Python side is lossless, its MATLAB side
carries skull absorption in matlab/skull2medium.m and fitPowerLawParamsMulti.m).

The solver's operator is ``L(u) + k~^2 u`` with the PML stretched by ``gamma = 1 + i sigma / k`` (laplacian.py), i.e. the time convention in which an
outgoing wave is ``e^{+ikx}``.  Such a wave decays along its way for ``Im(k~) > 0``, so a medium that ABSORBS has

    k~ = omega / c + i alpha,          alpha >= 0 in nepers per grid point,
    k~^2 = (omega / c)^2 - alpha^2  +  i * 2 (omega / c) alpha.

The library takes the two planes apart (``hn_residual_lossy``, ``hn_step_lossy``, ``hn_fgmres_cycle_lossy`` and, for adjoint-state gradients,
``hn_residual_vjp_lossy``, ``hn_fgmres_adjoint_cycle_lossy``, ``hn_adjoint_grad_lossy``): ``k_sq`` and ``k_sq_im >= 0``.  The other
sign (alpha < 0) amplifies: the float64 direct solve of a 32^2 ring phantom has an rms of 0.58 without loss, 0.39 at alpha = 0.1 and 7.2 at alpha = -0.1.
"""
from __future__ import annotations

import torch


def complex_k_sq(sos: torch.Tensor, alpha, omega: float = 1.0):
    """(k_sq, k_sq_im) of the medium with sound speed ``sos`` [B,1,H,W] and absorption ``alpha`` (a number or a tensor broadcastable to ``sos``, nepers
    per grid point; positive absorbs, see the module docstring for the sign): ``k_sq = (omega / sos)^2 - alpha^2`` and ``k_sq_im = 2 (omega / sos) alpha``,
    both in the dtype of ``sos``.  ``alpha = 0`` gives ``IterativeSolver.get_initials``' ``k_sq`` bit for bit and a plane of zeros."""
    if not isinstance(sos, torch.Tensor):
        raise TypeError("sos must be a tensor")
    alpha = torch.as_tensor(alpha, dtype=sos.dtype, device=sos.device)
    try:
        alpha = alpha.expand_as(sos)
    except RuntimeError as e:
        raise ValueError(f"alpha of shape {tuple(alpha.shape)} does not broadcast to sos {tuple(sos.shape)}") from e
    k = omega / sos
    # (omega / sos) ** 2 first, exactly as get_initials forms it: subtracting alpha^2 = 0 leaves its bits alone
    return (k ** 2 - alpha * alpha).contiguous(), (2.0 * k * alpha).contiguous()


def complex_k_sq_grads(g_k_sq: torch.Tensor, g_k_sq_im: torch.Tensor, sos: torch.Tensor, alpha, omega: float = 1.0):
    """The chain rule of ``complex_k_sq``, in the tensors' own dtype (float64 on the host in the tests, fp32 on the device in the backward pass of
    ``IterativeSolver.solve_implicit``): from dJ/dk_sq and dJ/dk_sq_im [B,1,H,W] to (dJ/dsos, dJ/dalpha), both [B,1,H,W] -- a caller whose ``alpha``
    was broadcast sums dJ/dalpha over the broadcast dimensions.  With k = omega / sos, k_sq = k^2 - alpha^2 and k_sq_im = 2 k alpha:

        dJ/dsos   = (2 k dJ/dk_sq + 2 alpha dJ/dk_sq_im) * (-omega / sos^2)
        dJ/dalpha = -2 alpha dJ/dk_sq + 2 k dJ/dk_sq_im"""
    alpha = torch.as_tensor(alpha, dtype=sos.dtype, device=sos.device).expand_as(sos)
    k = omega / sos
    g_sos = (2.0 * k * g_k_sq + 2.0 * alpha * g_k_sq_im) * (-omega / sos ** 2)
    g_alpha = -2.0 * alpha * g_k_sq + 2.0 * k * g_k_sq_im
    return g_sos, g_alpha
