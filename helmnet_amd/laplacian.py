"""Host-side mirror of the reference's spectral operator module.

Mirrors ``FastLaplacianWithPML`` (reference helmnet/spectral.py:246-363): same constructor,
same attribute names and tensor layouts (``kx, ky, kx_sq, ky_sq, ax, bx, ay, by`` as
``[1, N, N, 2]`` (re, im) fp32 parameters, ``sigma_x, sigma_y`` as ``[N, N]``; with a pair ``(H, W)`` as
``domain_size`` -- an extension, the reference assumes a square -- ``[1, H, W, 2]`` and ``[H, W]``, the x tables from the
1-D tables of length W, the y tables from those of length H), same
``forward(x[B, N, N, 2])`` and ``sigmas()``.  The tables are built exactly as the reference does
(float64 numpy, then cast); the arithmetic of ``forward`` runs in libhelmnet_hip.so
(``hn_laplacian``), which builds its own copy of the constants in C++ -- the GPU tests check
the two against each other.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn


def k_grid(n: int) -> np.ndarray:
    """spectral.py:126-127: 2*pi*fftfreq layout with the Nyquist bin kept at -pi."""
    k = 2 * np.pi * np.linspace(-0.5, 0.5, n, endpoint=False)
    return np.concatenate((k[n // 2:], k[: n // 2]))


def pml_profile(n: int, pml: int, sigma_max: float, k: float):
    """1-D sigma, a = -gamma'/gamma^3, b = 1/gamma^2 in float64 (spectral.py:298-363)."""
    i = np.arange(pml)
    outer = sigma_max * (np.abs(1 - i / pml) ** 2)
    sigma = np.zeros(n)
    sigma[:pml] = outer
    sigma[-pml:] = outer[::-1]
    prime = np.zeros(n)
    sp = -2 * sigma_max * (1 - i / pml) / pml
    prime[:pml] = sp
    prime[-pml:] = -sp[::-1]
    inv_gamma = 1.0 / (1.0 + (1j / k) * sigma)
    a = -((1j / k) * prime) * inv_gamma ** 3
    b = inv_gamma ** 2
    return sigma, a, b


def spectral_route(n: int, pfa: int = 1, mixed: int = 0):
    """(name, P, Q) of the kernels hn_set_domain picks for an n x n domain under the options 'spectral_pfa' and 'spectral_mixed' -- the rule of
    spec_build (hn_spectral.hip), whose outcome Engine.counter('spectral_route') reports as 1 .. 4.  n = P * Q, P odd, Q a power of two.
        'pow2'          P == 1: the power-of-two kernels
        'prime_factor'  P in (3, 5, 7), Q >= 16 (up to 512 for P = 3, 256 for 5 and 7) and spectral_pfa: k_spec_pfa<Q, P>
        'mixed'         any other P in [3, 127] with Q in [16, 512] and spectral_mixed: k_spec_line (runtime P)
        'dense'         everything else: the n x n operator
    Every multiple of 16 in [16, 2048] that is neither 'pow2' nor 'prime_factor' has P in [9, 127] and Q in {16, 32, 64, 128}; no size was taken
    out of the mixed rule after measurement (profiles/spectral_mixed_bench.txt)."""
    n = int(n)
    if n < 16 or n > 2048:
        raise ValueError(f"domain size {n} outside [16, 2048]")
    q = n & -n
    p = n // q
    if p == 1:
        return "pow2", p, q
    if pfa and p in (3, 5, 7) and 16 <= q <= (512 if p == 3 else 256):
        return "prime_factor", p, q
    if mixed and 3 <= p <= 127 and 16 <= q <= 512:
        return "mixed", p, q
    return "dense", p, q


def f64_route(n: int, f64_fft: int = 0):
    """The route of the float64 operator (hn_laplacian_f64, hn_residual_f64 and everything built on them) on an n x n domain under the option
    'f64_fft', context-free like ``spectral_route``: ('dense',) for 0, the circulant kernel at every size; ('fft', P, Q) for 1, the line transforms
    of hn_f64_fft.hip with n = P * Q, Q the largest power of two dividing n -- for every multiple of 16 in [16, 2048] P is odd in [1, 127] and Q
    in [16, 2048], so no legal size falls back.  Engine.counter('f64_route') reports the route the last call took as 1 / 2."""
    n, f64_fft = int(n), int(f64_fft)
    if n < 16 or n > 2048 or n % 16:
        raise ValueError(f"domain size {n} is not a multiple of 16 in [16, 2048]")
    if f64_fft not in (0, 1):
        raise ValueError(f"f64_fft must be 0 or 1 (got {f64_fft})")
    if not f64_fft:
        return ("dense",)
    q = n & -n
    return "fft", n // q, q


def adjoint_weight(n: int, pml: int, sigma_max: float, k: float) -> np.ndarray:
    """W[i, j] = gamma_y[i] * gamma_x[j] with gamma = 1 + i sigma / k, complex128 [n, n]: the diagonal similarity under which the PML operator is
    complex-symmetric up to its discretisation (A^T ~ W A W^-1, hence A^-H g ~ conj(W * A^-1 (conj(g) / W))).  Context-free like ``spectral_route``:
    hn_fgmres_adjoint_cycle holds the same table (and 1 / W) on the device, formed from the fp32 value of sigma and rounded once to fp32."""
    sigma, _, _ = pml_profile(int(n), int(pml), float(sigma_max), float(k))
    gamma = 1.0 + (1j / float(k)) * sigma
    return np.outer(gamma, gamma)


def domain_hw(domain_size):
    """(rows, columns) of a domain size given as an int (n x n) or a pair (H, W)."""
    if isinstance(domain_size, (tuple, list)):
        if len(domain_size) != 2:
            raise ValueError(f"a rectangular domain size is a pair (H, W), got {domain_size!r}")
        return int(domain_size[0]), int(domain_size[1])
    return int(domain_size), int(domain_size)


def spectral_route_rect(h: int, w: int):
    """('rectangular', (P_h, Q_h), (P_w, Q_w)): the factorisation hn_set_domain_rect uses for an h x w domain with h != w -- the rule of
    spec_rect_factor (hn_spectral_line.hip), reported by Engine.counter('spectral_route') as 5.  Each axis on its own: len = P * Q with Q the
    largest power of two dividing it, which for every multiple of 16 in [16, 2048] gives P odd in [1, 127] and Q in [16, 2048]; every such
    length runs by FFT (P = 1: a plain power-of-two transform) and neither option 'spectral_pfa' nor 'spectral_mixed' is read.  h == w is
    hn_set_domain itself: see ``spectral_route``."""
    h, w = int(h), int(w)
    if h == w:
        raise ValueError(f"{h} x {w} is a square domain: hn_set_domain_rect delegates it to hn_set_domain (spectral_route)")
    out = []
    for n in (h, w):
        if n < 16 or n > 2048 or n % 16:
            raise ValueError(f"domain size {h} x {w}: {n} is not a multiple of 16 in [16, 2048]")
        q = n & -n
        out.append((n // q, q))
    return "rectangular", out[0], out[1]


def _frozen(t: torch.Tensor) -> nn.Parameter:
    return nn.Parameter(t, requires_grad=False)


class FastLaplacianWithPML(nn.Module):
    def __init__(self, domain_size: int, PMLsize: int, k: float, sigma_max: float):
        super().__init__()
        self._engine = None
        self.init_variables(PMLsize, domain_size, sigma_max, k)

    def init_variables(self, PMLsize, domain_size, sigma_max, k):
        self.PMLsize, self.domain_size, self.sigma_max, self.k = PMLsize, domain_size, sigma_max, k
        h, w = domain_hw(domain_size)                      # one set of 1-D tables per axis, each normalised by its own length
        sigma_h, a_h, b_h = pml_profile(h, PMLsize, sigma_max, k)
        sigma_w, a_w, b_w = pml_profile(w, PMLsize, sigma_max, k)
        kh32 = torch.from_numpy(k_grid(h)).float()         # cast before squaring, as the reference does
        kw32 = torch.from_numpy(k_grid(w)).float()
        kx = kw32.view(1, 1, w, 1).expand(1, h, w, 1)      # varies along the LAST axis ("x" = W)
        ky = kh32.view(1, h, 1, 1).expand(1, h, w, 1)
        zero = torch.zeros(1, h, w, 1)
        self.kx = _frozen(torch.cat([zero, kx], -1).contiguous())            # i*kx
        self.ky = _frozen(torch.cat([zero, ky], -1).contiguous())
        self.kx_sq = _frozen(torch.cat([-kx.pow(2), zero], -1).contiguous())  # -kx^2
        self.ky_sq = _frozen(torch.cat([-ky.pow(2), zero], -1).contiguous())

        def pair(c, along_x):
            t = torch.from_numpy(np.stack([c.real, c.imag], -1)).float()     # [len, 2]
            t = t.view(1, 1, w, 2).expand(1, h, w, 2) if along_x else t.view(1, h, 1, 2).expand(1, h, w, 2)
            return _frozen(t.contiguous())

        self.ax, self.bx = pair(a_w, True), pair(b_w, True)
        self.ay, self.by = pair(a_h, False), pair(b_h, False)
        self.sigma_x = _frozen(torch.from_numpy(sigma_w).float().view(1, w).expand(h, w).contiguous())
        self.sigma_y = _frozen(torch.from_numpy(sigma_h).float().view(h, 1).expand(h, w).contiguous())

    def sigmas(self):
        return self.sigma_x, self.sigma_y

    def bind(self, engine):
        """Share the owning solver's engine (its hn_set_domain already matches this module)."""
        self._engine = engine

    def _get_engine(self, device):
        from .engine import Engine
        h, w = domain_hw(self.domain_size)
        tail = (int(self.PMLsize), float(self.sigma_max), float(self.k))
        if self._engine is None or self._engine.device != torch.device(device):
            self._engine = Engine(device)
        if h == w and self._engine.domain_key != (h,) + tail:
            self._engine.set_domain(h, *tail)
        elif h != w and self._engine.domain_key != ((h, w),) + tail:
            self._engine.set_domain_rect(h, w, *tail)
        return self._engine

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: [B, N, N, 2] (re, im last) -> L(x), same layout (spectral.py:251-262)."""
        eng = self._get_engine(x.device)
        nchw = x.permute(0, 3, 1, 2).contiguous()
        return eng.laplacian(nchw).permute(0, 2, 3, 1).contiguous()
