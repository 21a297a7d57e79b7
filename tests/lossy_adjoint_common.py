"""The lossy adjoint operator and the adjoint-state gradients of an absorbing medium: float64 references and seeded inputs shared by
tests/test_lossy_adjoint_host.py and tests/test_lossy_adjoint_gpu.py.

Nothing here comes from the code under test.  The adjoint operator is ``torch.autograd.grad`` through the float64 ``lossy_common.residual`` (the
oracle's Laplacian on the per-axis tables of tests/rect_common.py plus the complex pointwise term); the dense operator is
``O.assemble_helmholtz_matrix`` plus i diag(k_sq_im), as ``lossy_common.direct_solve`` builds it; the chain rule of the medium is autograd through the
formulas written out:  k = omega / c,  k_sq = k^2 - alpha^2,  k_sq_im = 2 k alpha.

With A u = L(u) + (k_sq + i k_sq_im) u, a real loss J, g = dJ/du as two real planes and A^H lam = g:
    A^H g       = L^H g + (k_sq - i k_sq_im) g
    dJ/dk_sq    = -(lam_re u_re + lam_im u_im)
    dJ/dk_sq_im = lam_re u_im - lam_im u_re
    dJ/dsrc     = lam
"""
import numpy as np
import torch

import lossy_common as LC
import rect_common as R
import spectral_probes as SP
from oracle import helmnet_oracle as O

PML, SIGMA_MAX, K, OMEGA = R.PML, R.SIGMA_MAX, R.K, 1.0
PROBES = SP.PROBES[:SP.ADJOINT_PROBES]       # noise and the two mode fields as cotangents
SQUARES = (16, 32, 48, 80, 112, 144, 208, 256)     # P = 1 (even and odd log2 Q), 3, 5, 7, 9, 13, and the headline size
RECTANGLES = ((32, 80), (48, 16))                  # P = 1 on one axis and 5 on the other; both axes the smallest lines


def adjoint_ref(g, k_sq, k_sq_im, h, w):
    """J^T g of the float64 ``LC.residual`` with respect to the wavefield (linear in it: any base point) -> [B,2,h,w] float64."""
    t = R.tables(h, w)
    wf = torch.zeros(g.shape, dtype=torch.float64, requires_grad=True)
    res = LC.residual(wf, k_sq.double(), k_sq_im.double(), torch.zeros(1, 2, h, w, dtype=torch.float64), t)
    return torch.autograd.grad(res, wf, g.double())[0]


_cases = {}


def adjoint_case(h, w):
    """Cotangents (the noise and mode probes of (h, w)), a seeded k_sq and k_sq_im (sample 1 with the amplifying sign) and the float64 A^H g.
    scale = max |L^H64(noise)|, bar = SP.BAR * (scale * peak(g) + peak(|k~^2| g)): the form of ``LC.forward_case`` without a source.  ``u``: the other
    field of <A u, g> = <u, A^H g>, a second noise plus the normalised expected A^H g (the construction of ``SP.adjoint_case``)."""
    key = (h, w)
    if key not in _cases:
        nb = len(PROBES)
        g = R.probe_batch(h, w)[:nb].contiguous()
        k_sq = R.seeded_k_sq(h, w, nb, 5100 + 3 * h + w)
        k_im = LC.seeded_k_sq_im(h, w, nb, 8100 + 3 * h + w)
        vjp = adjoint_ref(g, k_sq, k_im, h, w)
        gd, kr, ki = g.double(), k_sq.double(), k_im.double()
        conj_term = torch.cat([kr * gd[:, 0:1] + ki * gd[:, 1:2], kr * gd[:, 1:2] - ki * gd[:, 0:1]], 1)     # (k_sq - i k_sq_im) g
        scale = float((vjp[0] - conj_term[0]).abs().max())
        mag = torch.sqrt(kr ** 2 + ki ** 2) * gd.abs()
        u = (0.5 * R.noise_field(h, w, seed_offset=78)[None] + (vjp / scale).float()).contiguous()
        _cases[key] = dict(g=g, k_sq=k_sq, k_sq_im=k_im, vjp=vjp, scale=scale, bar=SP.BAR * (scale * SP.peak(g) + SP.peak(mag)), u=u)
    return _cases[key]


def lossless_bar(c):
    """The bar of the same cotangents for the lossless operator (k_sq_im = 0): SP.BAR * (scale * peak(g) + peak(k_sq g))."""
    return SP.BAR * (c["scale"] * SP.peak(c["g"]) + SP.peak(c["k_sq"].double() * c["g"].double()))


# ---- the medium and its chain rule -------------------------------------------------------------------------------------------------------------
def planes(sos, alpha, omega=OMEGA):
    """(k_sq, k_sq_im) by the formulas, in the dtype of ``sos`` (numpy or torch)."""
    k = omega / sos
    return k ** 2 - alpha ** 2, 2.0 * k * alpha


def chain_rule_ref(g_k_sq, g_k_sq_im, sos, alpha, omega=OMEGA):
    """(dJ/dsos, dJ/dalpha) by float64 autograd through ``planes``: J = <g_k_sq, k_sq> + <g_k_sq_im, k_sq_im>; ``alpha`` keeps its own shape, so a
    broadcast alpha receives the sum over the dimensions it was broadcast along."""
    s = sos.detach().double().clone().requires_grad_(True)
    a = torch.as_tensor(alpha, dtype=torch.float64).detach().clone().requires_grad_(True)
    k_sq, k_im = planes(s, a, omega)
    j = (g_k_sq.double() * k_sq).sum() + (g_k_sq_im.double() * k_im).sum()
    return torch.autograd.grad(j, (s, a))


# ---- dense float64 operator, solves and gradients ----------------------------------------------------------------------------------------------
def lossy_matrix(k_re, k_im):
    """The dense complex128 operator of one [n, n] medium given as two planes (fp32 values, as the device sees them)."""
    k_re, k_im = np.asarray(k_re, np.float32), np.asarray(k_im, np.float32)
    return O.assemble_helmholtz_matrix(k_re, PML, SIGMA_MAX, K) + 1j * np.diag(k_im.reshape(-1).astype(np.float64))


def np_complex(t):
    """A planar field [..., 2, n, n] or a stack of planar vectors [..., 2 P] as complex128 numpy [..., P]."""
    v = t.detach().double().cpu().numpy()
    if v.ndim >= 3 and v.shape[-3] == 2:
        v = v.reshape(*v.shape[:-3], -1)
    p = v.shape[-1] // 2
    return v[..., :p] + 1j * v[..., p:]


def scaled_field(shape, seed, norm):
    """A seeded real field [B, 2, n, n] (fp32 values) whose samples have the 2-norm ``norm``."""
    g = torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    g = g * (norm / torch.linalg.vector_norm(g.reshape(shape[0], -1), dim=1)).reshape(-1, 1, 1, 1)
    return g.float().contiguous()


_media = {}


def ring_problem(n, a0, b=2, uniform=False):
    """The issue's ring media: (sos, alpha) fp32 [b,1,n,n] -- alpha by ``LC.ring_alpha``, or a0 everywhere (``uniform``: what a number for
    ``absorption`` means) -- and the fp32 planes the device forms from them."""
    key = (n, a0, b, uniform)
    if key not in _media:
        sos, alpha = LC.ring_medium(n, a0, b=b)
        if uniform:
            alpha = torch.full_like(sos, a0)
        k_sq, k_im = planes(sos, alpha)
        _media[key] = dict(sos=sos, alpha=alpha, k_sq=k_sq.contiguous(), k_sq_im=k_im.contiguous())
    return _media[key]


def medium_matrix(sos, alpha):
    """The dense complex128 operator of the medium (sos, alpha) [n, n] float64, the planes formed in float64."""
    k_sq, k_im = planes(sos, alpha)
    return O.assemble_helmholtz_matrix(k_sq, PML, SIGMA_MAX, K) + 1j * np.diag(k_im.reshape(-1))


def loss64(M, sos_m, alpha_m, sos, alpha, src, rx, d):
    """J = 1/2 sum |u[rx] - d|^2 of the dense float64 solve on the medium (sos, alpha), from the operator M of the medium (sos_m, alpha_m): only
    the diagonal differs."""
    M = M.copy()
    i = np.arange(M.shape[0])
    (k0, i0), (k1, i1) = planes(sos_m, alpha_m), planes(sos, alpha)
    M[i, i] += ((k1 - k0) + 1j * (i1 - i0)).reshape(-1)
    u = np.linalg.solve(M, src).reshape(sos.shape)
    return 0.5 * float((np.abs(u[rx] - d) ** 2).sum())


_grad_refs = {}


def gradient_reference(n, a0, src, uniform=False):
    """Dense float64 adjoint-state gradients of the receiver-row loss J = 1/2 sum |u[rx] - d|^2 on the two media of ``ring_problem(n, a0)``;
    ``src`` complex [n * n] is the solver's source.  d is u's own row minus a seeded field of the source's 2-norm, so that the adjoint right-hand
    side is that field (the construction of test_adjoint_gpu._gradient_reference).  The medium is the float64 up-cast of the fp32 (sos, alpha)."""
    key = (n, a0, uniform)
    if key in _grad_refs:
        return _grad_refs[key]
    p = ring_problem(n, a0, uniform=uniform)
    rx = n // 2 + 4
    rng = np.random.default_rng(400 + n)
    ref = {"rx": rx, "d": [], "u": [], "lam": [], "g_k_sq": [], "g_k_sq_im": [], "g_sos": [], "g_alpha": [], "chain_sos": [], "chain_alpha": [], "M": []}
    for b in range(2):
        sos, alpha = p["sos"][b, 0].double().numpy(), p["alpha"][b, 0].double().numpy()
        M = medium_matrix(sos, alpha)
        u = np.linalg.solve(M, src).reshape(n, n)
        gt = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        gt *= np.linalg.norm(src) / np.linalg.norm(gt)
        g = np.zeros((n, n), np.complex128)
        g[rx] = gt
        lam = np.linalg.solve(M.conj().T, g.reshape(-1)).reshape(n, n)
        g_k = -(lam.real * u.real + lam.imag * u.imag)
        g_ki = lam.real * u.imag - lam.imag * u.real
        k = OMEGA / sos
        ref["d"].append(u[rx] - gt); ref["u"].append(u); ref["lam"].append(lam); ref["g_k_sq"].append(g_k); ref["g_k_sq_im"].append(g_ki)
        ref["M"].append(M)
        ref["g_sos"].append((2.0 * k * g_k + 2.0 * alpha * g_ki) * (-OMEGA / sos ** 2))
        ref["g_alpha"].append(-2.0 * alpha * g_k + 2.0 * k * g_ki)
        # |d g_sos| <= (2 k |d g_k| + 2 alpha |d g_ki|) omega / sos^2 and |d g_alpha| <= 2 alpha |d g_k| + 2 k |d g_ki|, the same bar on either
        ref["chain_sos"].append(float(((2.0 * k + 2.0 * np.abs(alpha)) * OMEGA / sos ** 2).max()))
        ref["chain_alpha"].append(float((2.0 * np.abs(alpha) + 2.0 * k).max()))
    ref["g_src"] = ref["lam"][0] + ref["lam"][1]                 # one source map shared by the batch
    _grad_refs[key] = ref
    return ref
