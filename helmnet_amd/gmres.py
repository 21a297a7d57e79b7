"""Matrix-free restarted GMRES on the SAME HIP Helmholtz operator the learned solver uses.

The reference's classical baseline is MATLAB's ``gmres`` on an explicitly assembled spectral PML
operator (matlab/spectral_gmres_solver.m:50-115).  Here the operator application
A u = L(u) + k_sq * u is libhelmnet_hip.so's fused residual kernel (``hn_residual`` with a zero
source); the Krylov bookkeeping runs on the device as batched matrix-vector products over one pre-allocated basis tensor,
with no host synchronisation inside a restart cycle (r4; the r3 version did modified Gram-Schmidt vector by vector, a
``torch.linalg.lstsq`` and a host read-back per inner iteration: 13 it/s on an operator that applies in 25 us).  All samples
of a batch are solved independently in lock step.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .engine import Medium, _require_no_grad


def _hessenberg_least_squares(H: np.ndarray, beta: np.ndarray):
    """Progressive Givens QR of the [B, m + 1, m] Hessenberg matrices (complex128, on the host: a few kilobytes once per restart
    cycle).  Returns (R, g, res) with R [B, m, m] upper triangular, g [B, m + 1] the rotated right-hand side beta * e_1 and
    res [B, m] = the residual 2-norm after 1 .. m inner iterations (= |g[j + 1]| after the j-th rotation)."""
    B, m1, m = H.shape
    R = H.copy()
    g = np.zeros((B, m1), dtype=np.complex128)
    g[:, 0] = beta
    res = np.zeros((B, m))
    for j in range(m):
        a, b = R[:, j, j].copy(), R[:, j + 1, j].copy()
        d = np.sqrt(np.abs(a) ** 2 + np.abs(b) ** 2)
        d = np.where(d == 0.0, 1.0, d)
        c, s_ = a / d, b / d                       # rotation [[conj(c), conj(s)], [-s, c]] zeroes R[j + 1, j]
        rj, rj1 = R[:, j, j:].copy(), R[:, j + 1, j:].copy()
        R[:, j, j:] = np.conj(c)[:, None] * rj + np.conj(s_)[:, None] * rj1
        R[:, j + 1, j:] = -s_[:, None] * rj + c[:, None] * rj1
        gj, gj1 = g[:, j].copy(), g[:, j + 1].copy()
        g[:, j] = np.conj(c) * gj + np.conj(s_) * gj1
        g[:, j + 1] = -s_ * gj + c * gj1
        res[:, j] = np.abs(g[:, j + 1])
    return R[:, :m, :], g, res


def _back_substitute(R: np.ndarray, g: np.ndarray, k: int) -> np.ndarray:
    """y [B, k] with R[:, :k, :k] y = g[:, :k] (upper triangular)."""
    B = R.shape[0]
    y = np.zeros((B, k), dtype=np.complex128)
    for i in range(k - 1, -1, -1):
        diag = np.where(R[:, i, i] == 0.0, 1.0, R[:, i, i])
        y[:, i] = (g[:, i] - np.einsum("bj,bj->b", R[:, i, i + 1:k], y[:, i + 1:k])) / diag
    return y


def drive_cycles(cycle, true_rmse, max_cycles: int, tol: float) -> dict:
    """The host loop of ``gmres(backend="hip")``, free of torch and of the library so that it is tested on the CPU with a scripted cycle.

    ``cycle()`` runs one restart cycle on the current iterate and returns ``(rmse [m + 1, B], k_used [B])`` as host arrays (the tables of
    ``hn_gmres_cycle``: row 0 the true RMSE at the start, row j the estimate after j inner iterations); ``true_rmse()`` returns the true
    residual RMSE [B] of the current iterate.  Per cycle the history gains rows 0 .. max(k_used), a sample's rows past its own ``k_used``
    repeating the value it stopped at.  Once every sample's estimate at its ``k_used`` is below ``tol`` the true residual is evaluated
    (the estimate comes from an fp32 Hessenberg matrix); it replaces the last history row, and the loop ends if it is below ``tol`` for
    every sample -- else the next cycle starts from it.  Returns history (list of [B] float32 arrays), tables (the per-cycle tables as they
    came), iterations (lock-step inner iterations: sum of max(k_used)), iterations_per_sample (int64 [B]: sum of k_used), cycles,
    true_checks and converged."""
    history, tables, its, per, converged, checks, cycles = [], [], 0, None, False, 0, 0
    for _ in range(int(max_cycles)):
        rm, ku = cycle()
        rm, ku = np.asarray(rm, dtype=np.float32), np.asarray(ku, dtype=np.int64)
        cycles += 1
        tables.append(rm)
        per = ku.copy() if per is None else per + ku
        kmax = int(ku.max())
        its += kmax
        cols = np.arange(rm.shape[1])
        for j in range(kmax + 1):
            history.append(rm[np.minimum(j, ku), cols].copy())
        if bool((rm[ku, cols] < tol).all()):
            t = np.asarray(true_rmse(), dtype=np.float32)
            checks += 1
            history[-1] = t
            if bool((t < tol).all()):
                converged = True
                break
    return {"history": history, "tables": tables, "iterations": its, "iterations_per_sample": per if per is not None else np.zeros(0, np.int64),
            "cycles": cycles, "true_checks": checks, "converged": converged}


def drive_refinement(cycle, max_cycles: int, tol: float) -> dict:
    """The host loop of ``gmres(backend="hip", refine=True)``, free of torch and of the library like ``drive_cycles``.

    ``cycle()`` runs one refinement step on the current float64 iterate and returns ``(rmse64 [B], rmse [m + 1, B], k_used [B])`` as host arrays
    (the outputs of ``hn_gmres_refine_cycle``: the TRUE float64 residual RMSE at the start of the step and the inner fp32 cycle's tables); they
    are read once per cycle.  The loop ends with the first cycle whose ``rmse64`` is below ``tol`` for every sample: that cycle is the final true
    check, it has updated nothing (its ``k_used`` is zero).  At most ``max_cycles`` calls are made, the checking one included.  Returns history
    (list of [B] float64 arrays: the true RMSE at the start of every cycle, the last one that of the returned iterate when converged), tables
    (the inner rmse tables as they came), iterations (lock-step inner iterations: sum of max(k_used)), iterations_per_sample (int64 [B]),
    cycles and converged."""
    history, tables, its, per, converged, cycles = [], [], 0, None, False, 0
    for _ in range(int(max_cycles)):
        r64, rm, ku = cycle()
        r64, rm, ku = np.asarray(r64, dtype=np.float64), np.asarray(rm, dtype=np.float32), np.asarray(ku, dtype=np.int64)
        cycles += 1
        history.append(r64.copy())
        tables.append(rm)
        per = ku.copy() if per is None else per + ku
        its += int(ku.max())
        if bool((r64 < tol).all()):
            converged = True
            break
    return {"history": history, "tables": tables, "iterations": its, "iterations_per_sample": per if per is not None else np.zeros(0, np.int64),
            "cycles": cycles, "converged": converged}


def unet_evaluations(cycles: int, restart: int, precond_iterations: int) -> int:
    """UNet evaluations a preconditioned solve of ``cycles`` cycles (a driver's count, a refinement's final checking cycle included) has enqueued:
    every cycle runs all ``restart`` inner steps in lock step for the whole batch, whatever stopped on the way, each with ``precond_iterations``
    iterations of the learned solver.  Zero without a preconditioner."""
    return int(cycles) * int(restart) * int(precond_iterations)


def default_precond_scale(source) -> float:
    """alpha of ``precondition="learned"`` when none is given: the root-mean-square 2-norm of the source maps [S,2,n,n], ||src||_F / sqrt(S), in
    float64 on the host -- the preconditioner's right-hand side alpha * v_k (|v_k| = 1) then has the magnitude the network was trained on."""
    src = np.asarray(source.detach().double().cpu().numpy() if isinstance(source, torch.Tensor) else source, dtype=np.float64)
    return float(np.sqrt((src ** 2).sum() / src.shape[0]))


def _hip_setup(solver, sos_maps, restart, x0, dtype, absorption=None, density=None):
    """What the HIP drivers start from: (engine, the Medium, rhs, the iterate x in ``dtype`` -- a copy of ``x0``, zeros without one --, basis, hess)."""
    _require_no_grad("gmres(backend='hip')", sos_maps, x0, absorption, density)
    eng = solver.engine()
    if absorption is None and density is None:
        k_sq, wf0 = solver.get_initials(sos_maps.float().contiguous())
        m = Medium(k_sq.contiguous())
    else:
        m, wf0 = solver._initials("gmres", sos_maps, absorption, density)
    rhs = solver.source.detach().float().contiguous()
    bsz, n = sos_maps.shape[0], sos_maps.shape[-1]
    x = (wf0 if x0 is None else x0.detach()).to(rhs.device, dtype).contiguous().clone()
    basis = torch.empty(bsz, restart + 1, 2 * n * n, dtype=torch.float32, device=rhs.device)
    hess = torch.empty(bsz, restart + 1, restart, 2, dtype=torch.float32, device=rhs.device)
    return eng, m, rhs, x, basis, hess


def _zbasis(m: Medium, precond, basis):
    """The flexible cycles' second basis; None where the plain cycle runs: a lossless medium without a preconditioner."""
    if precond is None and not m.kind:
        return None
    return torch.empty(basis.shape[0], basis.shape[1] - 1, basis.shape[2], dtype=torch.float32, device=basis.device)


def _gmres_refine(solver, sos_maps, restart, max_outer, tol, x0, inner_floor, precond=None, absorption=None):
    """``gmres(backend="hip", refine=True)`` and ``gmres_refine_lossy``: iterative refinement with the fp32 restart cycle as the inner solver
    (hn_gmres_refine_cycle).  The iterate, its true residual and the update are float64; one host synchronisation per cycle.  ``precond``
    (iterations, alpha): the flexible cycle (hn_fgmres_refine_cycle).  ``absorption``: the lossy operator (hn_fgmres_refine_cycle_lossy, with zero
    preconditioner iterations when ``precond`` is None)."""
    eng, m, rhs, x, basis, hess = _hip_setup(solver, sos_maps, restart, x0, torch.float64, absorption)
    bsz, dev = x.shape[0], x.device
    zbasis = _zbasis(m, precond, basis)
    iters, alpha = (0, 1.0) if precond is None else precond

    def cycle():
        if zbasis is None:
            rmse64, rmse, k_used = eng.gmres_refine_cycle(x, m.k_sq, rhs, restart, tol, inner_floor, basis, hess)
        else:
            rmse64, rmse, k_used = getattr(eng, "fgmres_refine_cycle" + m.kind)(x, *m.planes(), rhs, restart, tol, iters, alpha, inner_floor, basis, hess,
                                                                               zbasis)
        both = torch.cat([rmse64, rmse.reshape(-1).double(), k_used.double()]).cpu().numpy()          # the one synchronisation of the cycle
        eng.check_async_errors()
        n_tab = (restart + 1) * bsz
        return both[:bsz], both[bsz: bsz + n_tab].reshape(restart + 1, bsz), both[bsz + n_tab:].astype(np.int64)

    out = drive_refinement(cycle, max_outer, tol)
    # converged: the last cycle checked the returned iterate and wrote nothing; else its last update is still unchecked
    final = (torch.from_numpy(out["history"][-1]).to(dev) if out["converged"]
             else getattr(eng, "residual64" + m.kind)(x, *(p.double() for p in m.planes()), rhs.double(), False, True)[1])
    return {"wavefield": x, "residual_norm64": final, "residual_norms": [torch.from_numpy(h).to(dev) for h in out["history"]], "iterations": out["iterations"],
            "operator_applications": out["cycles"] * (restart + 1), "operator_applications64": out["cycles"], "converged": out["converged"],
            "iterations_per_sample": torch.from_numpy(out["iterations_per_sample"]), "cycle_tables": out["tables"], "cycles": out["cycles"],
            "unet_evaluations": unet_evaluations(out["cycles"], restart, iters)}


def gmres_refine_lossy(solver, sos_maps: torch.Tensor, absorption, restart: int = 20, max_outer: int = 400, tol: float = 1e-10,
                       x0: Optional[torch.Tensor] = None, inner_floor: float = 1e-6, precondition: Optional[str] = None, precond_iterations: int = 10,
                       precond_scale: Optional[float] = None):
    """GMRES to float64 accuracy on the LOSSY operator A u = L(u) + (k_sq + i k_sq_im) u (``absorption``: alpha, as in ``gmres``): the refinement of
    ``gmres(backend="hip", refine=True)`` on hn_fgmres_refine_cycle_lossy -- per cycle the float64 lossy residual (hn_residual_f64_lossy's), the fp32
    lossy cycle on the scaled correction equation (``precondition="learned"``: preconditioned by the lossy learned iteration; None: zero
    preconditioner iterations, plain refined GMRES) and x += s d in float64.  Returns the dictionary of the lossless refinement.  Square domains;
    no gradients."""
    if absorption is None:
        raise ValueError("gmres_refine_lossy needs absorption (a lossless medium is gmres(backend='hip', refine=True))")
    if precondition not in (None, "learned"):
        raise ValueError(f"unknown precondition {precondition!r} (choose None or 'learned')")
    if precondition is not None and int(precond_iterations) < 0:
        raise ValueError(f"precond_iterations must be >= 0 (got {precond_iterations})")
    solver._refuse_medium_grad("gmres64", False, sos_maps, absorption, x0)
    solver._require_square("gmres64 with absorption")
    precond = None
    if precondition is not None:
        precond = (int(precond_iterations), default_precond_scale(solver.source) if precond_scale is None else float(precond_scale))
    return _gmres_refine(solver, sos_maps, int(restart), int(max_outer), float(tol), x0, float(inner_floor), precond, absorption)


def _gmres_hip(solver, sos_maps, restart, max_outer, tol, x0, precond=None, absorption=None, density=None):
    """``gmres`` with the restart cycle as fused HIP launches (hn_gmres_cycle): one host synchronisation per cycle, every sample stopping on its own.
    ``precond`` (iterations, alpha): the flexible cycle (hn_fgmres_cycle).  ``absorption``: the lossy operator (hn_fgmres_cycle_lossy, with zero
    preconditioner iterations when ``precond`` is None).  ``density``: the variable-density operator (hn_fgmres_cycle_medium, likewise), with or
    without ``absorption``."""
    eng, m, rhs, x, basis, hess = _hip_setup(solver, sos_maps, restart, x0, torch.float32, absorption, density)
    bsz, dev = x.shape[0], x.device
    zbasis = _zbasis(m, precond, basis)
    iters, alpha = (0, 1.0) if precond is None else precond

    def cycle():
        if zbasis is None:
            rmse, k_used = eng.gmres_cycle(x, m.k_sq, rhs, restart, tol, basis, hess)
        else:
            rmse, k_used = getattr(eng, "fgmres_cycle" + m.kind)(x, *m.planes(), rhs, restart, tol, iters, alpha, basis, hess, zbasis)
        both = torch.cat([rmse.reshape(-1), k_used.float()]).cpu().numpy()          # the one synchronisation of the cycle
        eng.check_async_errors()
        return both[: (restart + 1) * bsz].reshape(restart + 1, bsz), both[(restart + 1) * bsz:].astype(np.int64)

    def true_rmse():
        return eng.rmse(getattr(eng, "residual" + m.kind)(x, *m.planes(), rhs)).cpu().numpy()

    out = drive_cycles(cycle, true_rmse, max_outer, tol)
    extra = {"cycles": out["cycles"]} if m.kind else {}
    return {"wavefield": x, "residual_norms": [torch.from_numpy(h).to(dev) for h in out["history"]], "iterations": out["iterations"],
            "operator_applications": out["cycles"] * (restart + 1) + out["true_checks"], "converged": out["converged"],
            "iterations_per_sample": torch.from_numpy(out["iterations_per_sample"]), "cycle_tables": out["tables"], **extra,
            "unet_evaluations": unet_evaluations(out["cycles"], restart, iters)}


def check_adjoint_rhs(solver, sos_maps, rhs):
    """The shapes ``gmres_adjoint`` takes, checked on the host before anything touches the device: ``sos_maps`` [B,1,n,n] and ``rhs`` [B or 1,2,n,n]
    on the solver's (square) n x n domain."""
    n = int(solver.hparams.domain_size)
    if not isinstance(sos_maps, torch.Tensor) or sos_maps.dim() != 4 or tuple(sos_maps.shape[1:]) != (1, n, n):
        raise ValueError(f"sos_maps must be [B, 1, {n}, {n}], got {tuple(getattr(sos_maps, 'shape', ()))}")
    b = int(sos_maps.shape[0])
    if not isinstance(rhs, torch.Tensor) or rhs.dim() != 4 or tuple(rhs.shape[1:]) != (2, n, n) or rhs.shape[0] not in (1, b):
        raise ValueError(f"the adjoint right-hand side must be [1 or {b}, 2, {n}, {n}], got {tuple(getattr(rhs, 'shape', ()))}")


def gmres_adjoint(solver, sos_maps: torch.Tensor, rhs: torch.Tensor, restart: int = 20, max_outer: int = 50, tol: float = 1e-4,
                  x0: Optional[torch.Tensor] = None, precondition: Optional[str] = None, precond_iterations: int = 10,
                  precond_scale: Optional[float] = None, backend: str = "hip", absorption=None, density=None):
    """Solve the ADJOINT system A^H lam = rhs for every map of ``sos_maps`` [B,1,n,n]: A u = L(u) + k_sq * u is the operator of ``gmres``, A^H its
    conjugate transpose (``hn_residual_vjp``), ``rhs`` [B or 1,2,n,n] a cotangent dJ/du as two real planes.  Restarted GMRES with the cycle fused
    on the device (hn_fgmres_adjoint_cycle), on the host loop of ``gmres(backend="hip")`` (``drive_cycles``): one synchronisation per cycle, every
    sample stopping on its own, and once every sample's estimate is below ``tol`` the TRUE residual ||rhs - A^H x|| (hn_residual_vjp) decides.

    ``precondition="learned"``: flexible GMRES with the learned iteration between the similarity weight W of ``laplacian.adjoint_weight`` --
    z_k = conj(W * M(conj(v_k) / W)), M = ``precond_iterations`` iterations of the network from rest on a right-hand side scaled by
    ``precond_scale`` (None: ``default_precond_scale(solver.source)``, the magnitude the network was trained on, as for the forward system).
    Returns the keys of ``gmres(backend="hip")`` -- ``wavefield`` is the adjoint state lam -- plus ``cycles``.  No gradients; there is no other
    backend.

    ``absorption`` (alpha, as in ``gmres``): the medium is lossy, A u = L(u) + (k_sq + i k_sq_im) u with both planes from
    ``helmnet_amd.absorption.complex_k_sq``, and A^H g = L^H(g) + (k_sq - i k_sq_im) g.  The cycles run on hn_fgmres_adjoint_cycle_lossy (the learned
    preconditioner is the lossy iteration between the same W) and the true-residual check on hn_residual_vjp_lossy.  None: the code path and the bits
    of before.

    ``density`` (rho, a tensor broadcastable to ``sos_maps``, as in ``gmres``): the operator is the variable-density one, with or without
    ``absorption``, A_rho^H g = L^H g - D_x^H(conj(b_x) q_x g) - D_y^H(conj(b_y) q_y g) + (k_sq - i k_sq_im) g with q = grad ln rho
    (``density.log_density_gradient``).  The cycles run on hn_fgmres_adjoint_cycle_medium -- the learned preconditioner is the variable-density
    iteration between the weight W / rho, which is why rho itself goes down and not only q -- and the true-residual check on hn_residual_vjp_medium.
    None: the code path and the bits of before."""
    if absorption is not None and backend != "hip":
        raise ValueError("absorption needs backend='hip' (gmres_adjoint has no other backend)")
    if density is not None and backend != "hip":
        raise ValueError("density needs backend='hip' (gmres_adjoint has no other backend)")
    if precondition not in (None, "learned"):
        raise ValueError(f"unknown precondition {precondition!r} (choose None or 'learned')")
    if precondition is not None and backend != "hip":
        raise ValueError("precondition='learned' needs backend='hip'")
    if backend != "hip":
        raise ValueError(f"gmres_adjoint has the 'hip' backend only (got {backend!r})")
    if precondition is not None and int(precond_iterations) < 0:
        raise ValueError(f"precond_iterations must be >= 0 (got {precond_iterations})")
    solver._require_square("gmres_adjoint")
    check_adjoint_rhs(solver, sos_maps, rhs)
    _require_no_grad("gmres_adjoint", sos_maps, rhs, x0, absorption, density)
    restart, max_outer, tol = int(restart), int(max_outer), float(tol)
    iters = 0 if precondition is None else int(precond_iterations)
    alpha = 1.0
    if precondition is not None:
        alpha = default_precond_scale(solver.source) if precond_scale is None else float(precond_scale)
    eng = solver.engine()
    sos_maps = sos_maps.to(eng.device).float().contiguous()
    if absorption is not None:
        from .absorption import complex_k_sq
        if isinstance(absorption, torch.Tensor):
            absorption = absorption.detach().to(eng.device, torch.float32)
        m = Medium(*complex_k_sq(sos_maps, absorption, solver.hparams.omega))
    else:
        m = Medium(solver.get_initials(sos_maps)[0].contiguous())
    rho = ()
    if density is not None:
        if not isinstance(density, torch.Tensor):
            raise TypeError("density must be a tensor broadcastable to the sound-speed maps")
        try:
            plane = density.detach().to(eng.device, torch.float32).expand_as(m.k_sq).contiguous()
        except RuntimeError as e:
            raise ValueError(f"density of shape {tuple(density.shape)} does not broadcast to {tuple(m.k_sq.shape)}") from e
        m = Medium(m.k_sq, m.k_sq_im, solver._rho_grad(plane, m.k_sq))
        rho = (plane,)        # the cycle's one argument behind the medium: the preconditioner's weight is W / rho
    rhs = rhs.detach().to(eng.device).float().contiguous()
    bsz, n, dev = sos_maps.shape[0], sos_maps.shape[-1], eng.device
    x = (torch.zeros(bsz, 2, n, n, device=dev) if x0 is None else x0.detach().to(dev, torch.float32)).contiguous().clone()
    basis = torch.empty(bsz, restart + 1, 2 * n * n, dtype=torch.float32, device=dev)
    zbasis = torch.empty(bsz, restart, 2 * n * n, dtype=torch.float32, device=dev)
    hess = torch.empty(bsz, restart + 1, restart, 2, dtype=torch.float32, device=dev)

    def cycle():
        rmse, k_used = getattr(eng, "fgmres_adjoint_cycle" + m.kind)(x, *m.planes(), *rho, rhs, restart, tol, iters, alpha, basis, zbasis, hess)
        both = torch.cat([rmse.reshape(-1), k_used.float()]).cpu().numpy()          # the one synchronisation of the cycle
        eng.check_async_errors()
        return both[: (restart + 1) * bsz].reshape(restart + 1, bsz), both[(restart + 1) * bsz:].astype(np.int64)

    def true_residual():
        return eng.rmse(rhs - getattr(eng, "residual_vjp" + m.kind)(x, *m.planes()))

    def true_rmse():
        return true_residual().cpu().numpy()

    out = drive_cycles(cycle, true_rmse, max_outer, tol)
    # converged: the last history row IS the true residual of the returned iterate; else its last update is still unchecked
    final = torch.from_numpy(out["history"][-1]).to(dev) if out["converged"] else true_residual()
    return {"wavefield": x, "residual_norms": [torch.from_numpy(h).to(dev) for h in out["history"]], "iterations": out["iterations"],
            "operator_applications": out["cycles"] * (restart + 1) + out["true_checks"] + (0 if out["converged"] else 1), "converged": out["converged"],
            "iterations_per_sample": torch.from_numpy(out["iterations_per_sample"]), "cycle_tables": out["tables"], "cycles": out["cycles"],
            "residual_norm": final, "unet_evaluations": unet_evaluations(out["cycles"], restart, iters)}


def gmres(solver, sos_maps: torch.Tensor, restart: int = 20, max_outer: int = 50, tol: float = 1e-4,
          x0: Optional[torch.Tensor] = None, backend: str = "torch", refine: bool = False, inner_floor: float = 1e-6,
          precondition: Optional[str] = None, precond_iterations: int = 10, precond_scale: Optional[float] = None, absorption=None,
          density=None):
    """Solve (L + k_sq) u = source for every map of ``sos_maps`` [B, 1, N, N] (the reference's classical baseline:
    matlab/spectral_gmres_solver.m:86-115, MATLAB's ``gmres`` with restarts).

    ``solver`` is a helmnet_amd.IterativeSolver on the GPU (its Laplacian tables and source are used).  Everything inside a
    restart cycle stays on the device, with no host read-back: the Krylov basis is ONE pre-allocated tensor in the operator's planar
    (re | im) layout, an Arnoldi step is the operator application (``hn_residual``), classical Gram-Schmidt with
    re-orthogonalisation as four batched matrix products over the basis, a norm and a scale.  The (m + 1) x m Hessenberg least-squares problem is
    solved ONCE per cycle (Givens rotations on the few kilobytes of H, read back at the end of the cycle), which also yields the
    residual norm after every inner iteration and the iteration at which the tolerance was met (the update then uses that
    many basis vectors: the GMRES iterate of that step).

    Returns dict(wavefield [B,2,N,N], residual_norms: list of [B] RMSE (hybridnet.py:295-297 definition) at the start of every
    cycle and after every inner iteration, iterations: inner iterations up to convergence, operator_applications: all of them).

    ``backend="hip"``: the same method with a restart cycle as a handful of fused HIP launches per inner step (hn_gmres_cycle), the
    Givens least-squares solve on the device and every sample stopping on its own; it adds ``iterations_per_sample`` (int64 [B]) and
    ``cycle_tables`` (the per-cycle rmse tables).

    ``backend="hip", refine=True``: GMRES to float64 accuracy at the fp32 cycle's speed -- classical iterative refinement with the fused fp32
    cycle as the inner solver (hn_gmres_refine_cycle).  Per cycle the true residual of the float64 iterate is evaluated in float64
    (hn_residual_f64's operator), the fp32 cycle solves the scaled correction equation A d = r / s from d = 0 to ``max(tol / s, inner_floor)``,
    and x += s d in float64.  ``tol`` is then a float64 RMSE; ``wavefield`` comes back float64, ``residual_norms`` is the list of TRUE float64
    RMSEs [B] at the start of every cycle, ``residual_norm64`` [B] that of the returned iterate, ``max_outer`` bounds the cycles, the
    final checking one included; ``x0`` may be fp32 (a learned solve's wavefield) or float64.

    ``backend="hip", precondition="learned"`` (with or without ``refine``): flexible GMRES with the learned solver as right preconditioner
    (hn_fgmres_cycle / hn_fgmres_refine_cycle) -- per inner step ``precond_iterations`` iterations of the solver's network on A z = alpha v_k from
    rest, z_k = wf / alpha.  ``precond_scale`` is alpha; None: ``default_precond_scale(solver.source)``.  The result gains ``unet_evaluations``
    (cycles x restart x precond_iterations, all enqueued in lock step; 0 without a preconditioner).  ``precondition=None`` is the code path and the
    bits of before.

    ``absorption`` (alpha in nepers per grid point, a number or a tensor broadcastable to ``sos_maps``; helmnet_amd.absorption): the medium is lossy,
    k~ = omega / sos + i alpha, and the cycles run on hn_fgmres_cycle_lossy.  ``backend="hip"`` with ``precondition`` None or "learned"; the torch
    backend raises ValueError, ``refine=True`` NotImplementedError (the float64 lossy refinement is ``gmres_refine_lossy``).  The result gains ``cycles``.  None: the code
    path and the bits of before.

    ``density`` (rho, a tensor broadcastable to ``sos_maps``; helmnet_amd.density): the cycles run on the variable-density operator
    (hn_fgmres_cycle_medium), with or without ``absorption``.  ``backend="hip"`` with ``precondition`` None or "learned"; the torch backend raises
    ValueError, ``refine=True`` NotImplementedError (the operator has no float64 counterpart).  The result gains ``cycles``.  None: the code path and
    the bits of before."""
    if density is not None:
        if backend != "hip":
            raise ValueError("density needs backend='hip' (the torch backend has the constant-density operator only)")
        if refine:
            raise NotImplementedError("gmres(refine=True) is not implemented with density: the variable-density operator has no float64 residual")
        solver._refuse_medium_grad("gmres", True, sos_maps, x0, absorption, density)
    if absorption is not None:
        if backend != "hip":
            raise ValueError("absorption needs backend='hip' (the torch backend has the lossless operator only)")
        if refine:
            raise NotImplementedError("gmres(refine=True) is not implemented with absorption: the float64 lossy refinement is gmres_refine_lossy "
                                      "(IterativeSolver.gmres64(absorption=...))")
    if refine and backend != "hip":
        raise ValueError("refine=True needs backend='hip'")
    if precondition not in (None, "learned"):
        raise ValueError(f"unknown precondition {precondition!r} (choose None or 'learned')")
    if precondition is not None and backend != "hip":
        raise ValueError("precondition='learned' needs backend='hip'")
    precond = None
    if precondition is not None:
        if int(precond_iterations) < 0:
            raise ValueError(f"precond_iterations must be >= 0 (got {precond_iterations})")
        _require_no_grad("gmres(backend='hip')", sos_maps, x0)
        precond = (int(precond_iterations), default_precond_scale(solver.source) if precond_scale is None else float(precond_scale))
    if backend == "hip" and refine:
        return _gmres_refine(solver, sos_maps, int(restart), int(max_outer), float(tol), x0, float(inner_floor), precond)
    if backend == "hip":
        return _gmres_hip(solver, sos_maps, int(restart), int(max_outer), float(tol), x0, precond, absorption, density)
    if backend != "torch":
        raise ValueError(f"unknown GMRES backend {backend!r} (choose 'torch' or 'hip')")
    eng = solver.engine()
    sos_maps = sos_maps.float().contiguous()
    k_sq, wf0 = solver.get_initials(sos_maps)
    k_sq = k_sq.contiguous()
    b_f = solver.source.detach().float()
    bsz, n = sos_maps.shape[0], sos_maps.shape[-1]
    b_f = b_f.expand(bsz, -1, -1, -1).contiguous() if b_f.shape[0] == 1 else b_f.contiguous()
    zero_src = torch.zeros_like(b_f[:1])
    P2 = 2 * n * n                       # a field as ONE real vector [re plane | im plane] -- the operator's own planar layout
    npix = float(P2)
    dev = b_f.device
    c = 512 if P2 % 512 == 0 else P2     # the basis is stored in S chunks of c entries: a product over the basis is then a batch of
    S = P2 // c                          # B * S small matrix products (split-K by layout), which fills the chip; one [k + 1, 2 N^2]
                                         # product per sample runs on a handful of workgroups (measured 3.6 ms per Arnoldi step)

    def apply_a(v):                      # v: [B, 2 N^2]
        return eng.residual(v.reshape(bsz, 2, n, n).contiguous(), k_sq, zero_src).reshape(bsz, P2)

    def rot(v):                          # multiplication by i in the planar layout: (re, im) -> (-im, re)
        return torch.cat([-v[:, P2 // 2:], v[:, : P2 // 2]], 1)

    x = (wf0 if x0 is None else x0.float()).contiguous().reshape(bsz, P2).clone()
    rhs = b_f.reshape(bsz, P2)
    V = torch.empty(bsz, S, restart + 1, c, dtype=torch.float32, device=dev)
    H = torch.zeros(bsz, restart + 1, restart, 2, dtype=torch.float32, device=dev)      # (re, im)
    tiny = 1e-30

    def project(w, k):
        """h_i = <v_i, w> (complex, conj on v) for i <= k as [B, k + 1, 2], and w - sum_i h_i v_i."""
        Vk = V[:, :, : k + 1].reshape(bsz * S, k + 1, c)
        W2 = torch.stack([w, -rot(w)], -1).reshape(bsz * S, c, 2)          # columns: w and -i w  ->  (re, im) of conj(v) . w
        h = torch.bmm(Vk, W2).reshape(bsz, S, k + 1, 2).sum(1)             # [B, k + 1, 2]
        hh = h.unsqueeze(1).expand(bsz, S, k + 1, 2).reshape(bsz * S, k + 1, 2)
        ab = torch.bmm(Vk.transpose(1, 2), hh).reshape(bsz, P2, 2)          # sum_i re(h_i) v_i and sum_i im(h_i) v_i
        return h, w - ab[..., 0] - rot(ab[..., 1])

    history, its, applications, converged = [], 0, 0, False
    for _ in range(max_outer):
        r = rhs - apply_a(x)
        applications += 1
        beta = torch.linalg.vector_norm(r, dim=1)                  # [B]
        V[:, :, 0] = (r / beta.clamp_min(tiny).unsqueeze(1)).reshape(bsz, S, c)
        H.zero_()
        for k in range(restart):                                   # Arnoldi: no host synchronisation in here
            w = apply_a(V[:, :, k].reshape(bsz, P2))
            h, w = project(w, k)
            h2, w = project(w, k)                                  # second pass: classical Gram-Schmidt loses orthogonality in fp32
            hn = torch.linalg.vector_norm(w, dim=1)
            H[:, : k + 1, k] = h + h2
            H[:, k + 1, k, 0] = hn
            V[:, :, k + 1] = (w / hn.clamp_min(tiny).unsqueeze(1)).reshape(bsz, S, c)
        applications += restart
        # ---- once per cycle: the small least-squares problem, on the host in float64 ----
        beta_h = beta.double().cpu().numpy()
        Hh = H.double().cpu().numpy()
        R, g, res = _hessenberg_least_squares(Hh[..., 0] + 1j * Hh[..., 1], beta_h)
        rm = np.concatenate([beta_h[:, None], res], 1) / np.sqrt(npix)          # RMSE before the cycle and after 1 .. m iterations
        below = np.nonzero(rm.max(0) < tol)[0]
        k_used = int(below[0]) if below.size else restart
        history += [torch.from_numpy(rm[:, j].astype(np.float32)).to(dev) for j in range(k_used + 1)]
        its += k_used
        if k_used > 0:
            y = _back_substitute(R, g, k_used)
            yy = torch.from_numpy(np.stack([y.real, y.imag], -1).astype(np.float32)).to(dev)       # [B, k_used, 2]
            Vk = V[:, :, :k_used].reshape(bsz * S, k_used, c)
            ab = torch.bmm(Vk.transpose(1, 2), yy.unsqueeze(1).expand(bsz, S, k_used, 2).reshape(bsz * S, k_used, 2)).reshape(bsz, P2, 2)
            x = x + ab[..., 0] + rot(ab[..., 1])
        if below.size:
            # the Givens estimate comes from a Hessenberg matrix built in fp32: before reporting convergence, apply the operator once more and check the TRUE
            # residual of the returned wavefield; if it is not below the tolerance the next cycle starts from it (r is recomputed at its top)
            true_rm = torch.linalg.vector_norm(rhs - apply_a(x), dim=1) / float(np.sqrt(npix))
            applications += 1
            history[-1] = true_rm
            if float(true_rm.max()) < tol:
                converged = True
                break
    wavefield = x.reshape(bsz, 2, n, n).contiguous()
    return {"wavefield": wavefield, "residual_norms": history, "iterations": its, "operator_applications": applications, "converged": converged}
