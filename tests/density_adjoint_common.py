"""The adjoint of the variable-density operator and its adjoint-state gradients: float64 references and seeded inputs shared by
tests/test_density_adjoint_host.py and tests/test_density_adjoint_gpu.py.

Nothing here comes from the code under test.  The adjoint operator is ``torch.autograd.grad`` through the float64 ``density_common.residual``; the
dense operator is ``lossy_adjoint_common.medium_matrix`` (the planes formed in float64 from sos and alpha) minus the density term of
``density_common.medium_matrix``, restated here without the fp32 rounding of q so that a central difference can move q by 1e-6; the chain from q to
rho is autograd through a torch restatement of ``density_common.log_gradient``.

With A_rho u = L(u) - b_x q_x D_x u - b_y q_y D_y u + (k_sq + i k_sq_im) u = src, a real loss J and A_rho^H lam = dJ/du:
    dJ/dk_sq, dJ/dk_sq_im, dJ/dsrc     as for the lossy operator (lossy_adjoint_common)
    dJ/dq_x = Re(conj(lam) b_x D_x u),   dJ/dq_y = Re(conj(lam) b_y D_y u)
    dJ/dln rho = -(G_x dJ/dq_x + G_y dJ/dq_y),   dJ/drho = dJ/dln rho / rho          (G: q = G ln rho per axis, real and antisymmetric)
"""
import numpy as np
import torch

import density_common as DC
import lossy_adjoint_common as LA
import rect_common as R
import spectral_probes as SP
from oracle import helmnet_oracle as O


def adjoint_ref(g, k_sq, k_sq_im, q, h, w):
    """J^T g of the float64 ``DC.residual`` with respect to the wavefield (linear in it: any base point) -> [B,2,h,w] float64; ``k_sq_im`` may be
    None."""
    t = R.tables(h, w)
    wf = torch.zeros(g.shape, dtype=torch.float64, requires_grad=True)
    res = DC.residual(wf, k_sq.double(), None if k_sq_im is None else k_sq_im.double(), q.double(), torch.zeros(1, 2, h, w, dtype=torch.float64), t)
    return torch.autograd.grad(res, wf, g.double())[0]


_cases = {}


def adjoint_case(h, w):
    """``LA.adjoint_case(h, w)`` (cotangents, k_sq, k_sq_im, the second field u) plus ``DC.seeded_q`` and the float64 A_rho^H g with k_sq_im
    (``vjp_m``) and without (``vjp_d``).  Bars: that case's lossy (lossless) bar plus SP.BAR * density_share(g, q, t), the way ``DC.forward_case``
    widens the forward bar."""
    key = (h, w)
    if key not in _cases:
        c = dict(LA.adjoint_case(h, w))
        q = DC.seeded_q(h, w, c["g"].shape[0])
        share = SP.BAR * DC.density_share(c["g"], q, R.tables(h, w))
        c.update(q=q, share=share, vjp_m=adjoint_ref(c["g"], c["k_sq"], c["k_sq_im"], q, h, w), vjp_d=adjoint_ref(c["g"], c["k_sq"], None, q, h, w),
                 bar_m=c["bar"] + share, bar_d=LA.lossless_bar(c) + share)
        _cases[key] = c
    return _cases[key]


# ---- q = G ln rho, restated in torch so that autograd gives the chain to rho ------------------------------------------------------------------
def log_gradient_torch(rho):
    """``DC.log_gradient`` in torch float64, differentiable: rho [B,1,H,W] -> q [B,2,H,W] (no rounding to fp32)."""
    ln = rho.double().log()
    h, w = ln.shape[-2:]
    kx, ky = torch.from_numpy(O.k_grid_1d(w)).reshape(1, 1, 1, w), torch.from_numpy(O.k_grid_1d(h)).reshape(1, 1, h, 1)
    qx = torch.fft.ifft(1j * kx * torch.fft.fft(ln, dim=3), dim=3).real
    qy = torch.fft.ifft(1j * ky * torch.fft.fft(ln, dim=2), dim=2).real
    return torch.cat([qx, qy], 1)


def rho_chain_ref(g_q, rho):
    """dJ/drho in rho's own shape by float64 autograd through ``log_gradient_torch``: J = <g_q, q(rho)>; a rho that was broadcast along the batch
    receives the sum over it."""
    r = rho.detach().double().clone().requires_grad_(True)
    q = log_gradient_torch(r.expand(g_q.shape[0], *r.shape[1:]))
    return torch.autograd.grad((g_q.double() * q).sum(), r)[0]


def log_gradient_matrix(n):
    """G of one axis, real [n, n]: q = G ln rho along that axis (the real part of idft diag(i k) dft on ``O.k_grid_1d``)."""
    k = O.k_grid_1d(n)
    return np.fft.ifft(1j * k[:, None] * np.fft.fft(np.eye(n), axis=0), axis=0).real


# ---- dense float64 operator ------------------------------------------------------------------------------------------------------------------
def b_profile(n):
    """b = 1 / gamma^2 of one axis, rounded to fp32 as ``DC.medium_matrix`` rounds it."""
    _, _, b = O.pml_profiles(n, R.PML, R.SIGMA_MAX, R.K)
    return b.real.astype(np.float32).astype(np.float64) + 1j * b.imag.astype(np.float32).astype(np.float64)


def density_matrix(q):
    """What A_rho adds to the constant-density matrix for q [2, n, n] float64 (NOT rounded): -(b_x q_x) D_x - (b_y q_y) D_y on the row-major field;
    linear in q."""
    q = np.asarray(q, np.float64)
    n = q.shape[-1]
    b = b_profile(n)
    bx = np.broadcast_to(b[None, :], (n, n)).reshape(-1)
    by = np.broadcast_to(b[:, None], (n, n)).reshape(-1)
    d1, eye = DC.d1_matrix(n), np.eye(n)
    return -(bx * q[0].reshape(-1))[:, None] * np.kron(eye, d1) - (by * q[1].reshape(-1))[:, None] * np.kron(d1, eye)


def first_derivatives_dense(u):
    """(b_x D_x u, b_y D_y u) of a complex [n, n] field with the matrices of ``density_matrix``."""
    n = u.shape[-1]
    b, d1 = b_profile(n), DC.d1_matrix(n)
    return b[None, :] * (u @ d1.T), b[:, None] * (d1 @ u)


_media = {}


def ring_problem(n, a0, b=2):
    """The three-map ring media: ``LA.ring_problem(n, a0)`` (sos, alpha, the fp32 planes) plus rho = ``DC.ring_density(sos)`` fp32, q fp32 =
    ``DC.log_gradient(rho)`` (what the device is handed) and q64, the same gradient without the rounding."""
    key = (n, a0, b)
    if key not in _media:
        p = dict(LA.ring_problem(n, a0, b=b))
        rho = DC.ring_density(p["sos"]).float().contiguous()
        p.update(rho=rho, q=DC.log_gradient(rho.numpy()), q64=log_gradient_torch(rho).numpy())
        _media[key] = p
    return _media[key]


def loss64(M, q_m, q, src, rx, d):
    """J = 1/2 sum |u[rx] - d|^2 of the dense float64 solve on the medium whose q is ``q`` [2, n, n], from the operator M of the same medium with
    ``q_m``: the matrix is linear in q."""
    n = q.shape[-1]
    u = np.linalg.solve(M + density_matrix(np.asarray(q, np.float64) - np.asarray(q_m, np.float64)), src).reshape(n, n)
    return 0.5 * float((np.abs(u[rx] - d) ** 2).sum())


_grad_refs = {}


def gradient_reference(n, a0, src, exact_q=False):
    """``LA.gradient_reference`` on the three-map ring media: dense float64 adjoint-state gradients of the receiver-row loss, with the density term in
    the operator, plus dJ/dq (``g_q`` [2, n, n]) and dJ/drho (``g_rho``).  ``exact_q``: the operator takes q64 (for central differences in float64)
    instead of the fp32 q the device is handed.  Chain factors, each a bound on |d gradient| / (4e-4 max|lam| max|u|), the error budget of the
    two solves (2e-4 of either):
        chain_sos, chain_alpha   as ``LA.gradient_reference``
        chain_q    = max|b| * ||D||_inf: dJ/dq = Re(conj(lam) b D u), |b D u| <= max|b| ||D||_inf max|u| and |b D du| <= max|b| ||D||_inf max|du|
        chain_rho  = chain_q * (||G_x||_inf + ||G_y||_inf) / min(rho): dJ/drho = -(G_x dJ/dq_x + G_y dJ/dq_y) / rho
    with || ||_inf the largest absolute row sum."""
    key = (n, a0, exact_q)
    if key in _grad_refs:
        return _grad_refs[key]
    p = ring_problem(n, a0)
    rx = n // 2 + 4
    rng = np.random.default_rng(400 + n)
    d_inf = float(np.abs(DC.d1_matrix(n)).sum(1).max())
    g_inf = float(np.abs(log_gradient_matrix(n)).sum(1).max())
    b_max = float(np.abs(b_profile(n)).max())
    names = ("d", "u", "lam", "g_k_sq", "g_k_sq_im", "g_sos", "g_alpha", "g_q", "g_rho", "chain_sos", "chain_alpha", "chain_q", "chain_rho", "M", "q")
    ref = {"rx": rx, **{k: [] for k in names}}
    for b in range(2):
        sos, alpha = p["sos"][b, 0].double().numpy(), p["alpha"][b, 0].double().numpy()
        rho = p["rho"][b, 0].double().numpy()
        q = p["q64"][b] if exact_q else p["q"][b].double().numpy()
        M = LA.medium_matrix(sos, alpha) + density_matrix(q)
        u = np.linalg.solve(M, src).reshape(n, n)
        gt = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        gt *= np.linalg.norm(src) / np.linalg.norm(gt)
        g = np.zeros((n, n), np.complex128)
        g[rx] = gt
        lam = np.linalg.solve(M.conj().T, g.reshape(-1)).reshape(n, n)
        g_k = -(lam.real * u.real + lam.imag * u.imag)
        g_ki = lam.real * u.imag - lam.imag * u.real
        dx, dy = first_derivatives_dense(u)
        g_q = np.stack([(np.conj(lam) * dx).real, (np.conj(lam) * dy).real])
        g_rho = rho_chain_ref(torch.from_numpy(g_q)[None], p["rho"][b:b + 1])[0, 0].numpy()
        k = LA.OMEGA / sos
        for name, v in (("d", u[rx] - gt), ("u", u), ("lam", lam), ("g_k_sq", g_k), ("g_k_sq_im", g_ki), ("M", M), ("q", q), ("g_q", g_q), ("g_rho", g_rho),
                        ("g_sos", (2.0 * k * g_k + 2.0 * alpha * g_ki) * (-LA.OMEGA / sos ** 2)), ("g_alpha", -2.0 * alpha * g_k + 2.0 * k * g_ki),
                        ("chain_sos", float(((2.0 * k + 2.0 * np.abs(alpha)) * LA.OMEGA / sos ** 2).max())),
                        ("chain_alpha", float((2.0 * np.abs(alpha) + 2.0 * k).max())), ("chain_q", b_max * d_inf),
                        ("chain_rho", b_max * d_inf * 2.0 * g_inf / float(rho.min()))):
            ref[name].append(v)
    ref["g_src"] = ref["lam"][0] + ref["lam"][1]                 # one source map shared by the batch
    _grad_refs[key] = ref
    return ref


# ---- the similarity weight of the learned preconditioner ---------------------------------------------------------------------------------------
def similarity_table(n):
    """For sample 0 of ``DC.ring_medium(n)`` (lossless) and X in (W, W / rho, W rho), W[i, j] = gamma_y[i] gamma_x[j] from the oracle's profile:
    {name: (||A^T - X A X^-1||_F / ||A||_F, ||A^H M - I||_2)} with M = conj(X A^-1 X^-1 conj(.)) built from the exact inverse, plus max|q|."""
    sos, rho, q = DC.ring_medium(n)
    A = DC.medium_matrix(((1.0 / sos[0, 0]) ** 2).numpy(), None, q[0].numpy())
    sigma, _, _ = O.pml_profiles(n, R.PML, R.SIGMA_MAX, R.K)
    gamma = 1.0 + 1j * sigma / R.K
    W = (gamma[:, None] * gamma[None, :]).reshape(-1)
    r = rho[0, 0].double().numpy().reshape(-1)
    Ainv = np.linalg.inv(A)
    out = {"max|q|": float(q[0].abs().max())}
    for name, x in (("W", W), ("W/rho", W / r), ("W*rho", W * r)):
        defect = float(np.linalg.norm(A.T - (x[:, None] * A) / x[None, :]) / np.linalg.norm(A))
        Mmat = np.conj((x[:, None] * Ainv) / x[None, :])          # z = conj(X A^-1 X^-1 conj(v))  <=>  z = conj(X A^-1 X^-1) v
        out[name] = (defect, float(np.linalg.norm(A.conj().T @ Mmat - np.eye(n * n), 2)))
    return out
