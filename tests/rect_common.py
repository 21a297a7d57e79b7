"""Rectangular (H x W) domains: the tables object the oracle needs, probes, float64 references and seeded inputs shared by
tests/test_rect_host.py and tests/test_rect_gpu.py.

The oracle's ``laplacian_nhwc``, ``get_residual``, ``unet_forward`` and ``single_step`` are shape-agnostic: they need a tables object with
``kx, ky, kx_sq, ky_sq, ax, bx, ay, by`` as [1, H, W, 2] and ``sigmas`` as [2, H, W].  ``RectTables`` builds it from ``O.k_grid_1d`` and
``O.pml_profiles``, one call per axis (the reference's formulas taken per axis, spectral.py:126-146, 298-363): the x tables vary along the last
axis with length W, the y tables along the first with length H, each axis normalised by its own length; k is cast to fp32 before squaring, as
``O.SpectralTables`` does.  tests/test_rect_host.py pins it: equal to ``O.SpectralTables`` at H == W, and equal to M_H U + U M_W^T in float64.

Probes are those of tests/spectral_probes.py built for (H, W); the bar is the same, 1e-5 of the operator's scale.
"""
import math

import numpy as np
import torch

import spectral_probes as SP
from oracle import helmnet_oracle as O

PML, SIGMA_MAX, K = SP.PML, SP.SIGMA_MAX, SP.K
DOMAIN = SP.DOMAIN
PROBES = SP.PROBES


class RectTables:
    def __init__(self, h: int, w: int, pml: int = PML, sigma_max: float = SIGMA_MAX, k: float = K, dtype=torch.float32):
        self.h, self.w = h, w
        kh, kw = O.k_grid_1d(h), O.k_grid_1d(w)
        sig_h, a_h, b_h = O.pml_profiles(h, pml, sigma_max, k)
        sig_w, a_w, b_w = O.pml_profiles(w, pml, sigma_max, k)
        kx2d, ky2d = np.meshgrid(kw, kh)                    # [h, w]: kx[i, j] = kw[j]; ky[i, j] = kh[i]
        kx32 = torch.from_numpy(kx2d).float()               # cast to float32 before squaring (spectral.py:274-277)
        ky32 = torch.from_numpy(ky2d).float()
        z = torch.zeros_like(kx32)

        def ri(re, im):
            return torch.stack([re, im], dim=-1).unsqueeze(0).to(dtype)

        def c2t(c):
            return ri(torch.from_numpy(np.real(c).copy()).float(), torch.from_numpy(np.imag(c).copy()).float())

        self.kx, self.ky = ri(z, kx32), ri(z, ky32)
        self.kx_sq, self.ky_sq = ri(-(kx32 ** 2), z), ri(-(ky32 ** 2), z)
        sx, sy = np.meshgrid(sig_w, sig_h)                  # sigma_x[i, j] = sigma_w[j]; sigma_y[i, j] = sigma_h[i]
        ax2, ay2 = np.meshgrid(a_w, a_h)
        bx2, by2 = np.meshgrid(b_w, b_h)
        self.ax, self.bx, self.ay, self.by = c2t(ax2), c2t(bx2), c2t(ay2), c2t(by2)
        self.sigma_x = torch.from_numpy(sx).float().to(dtype)
        self.sigma_y = torch.from_numpy(sy).float().to(dtype)
        self.sigmas = torch.stack([self.sigma_x, self.sigma_y], 0)


_tables = {}


def tables(h, w, domain=DOMAIN, dtype=torch.float64):
    key = (h, w, domain, dtype)
    if key not in _tables:
        _tables[key] = RectTables(h, w, *domain, dtype=dtype)
    return _tables[key]


# ---- the factorisation of one axis (helmnet_amd.laplacian.spectral_route_axis restated: the tests must not take it from the code under test) ----
def factor(length):
    """(P, Q): length = P * Q, Q the largest power of two that divides it."""
    q = 1
    while length % (2 * q) == 0:
        q *= 2
    return length // q, q


def state_len(h, w, depth=4):
    return sum((h >> d) * (w >> d) for d in range(depth))


def unflatten_states(flat, h, w, depth=4):
    out, o = [], 0
    for d in range(depth):
        m = (h >> d) * (w >> d)
        out.append(flat[:, :, o:o + m].reshape(flat.shape[0], flat.shape[1], h >> d, w >> d))
        o += m
    return out


# ---- probes ------------------------------------------------------------------------------------------------------------------------------------
def mode_indices(length):
    """SP.mode_indices of that axis' length plus that axis' P, Q, Q - 1, Q + 1."""
    p, q = factor(length)
    out = list(SP.mode_indices(length))
    for j in (p, q, q - 1, q + 1):
        if j % length not in out:
            out.append(j % length)
    return out


def mode_field(h, w, along_y=False):
    """modes_x: row i carries exp(i (2 pi j_i x / w + 0.37 i)); modes_y: column i carries exp(i (2 pi j_i y / h + 0.37 i))."""
    length, lines = (h, w) if along_y else (w, h)
    js = np.asarray(mode_indices(length), dtype=np.int64)
    line = np.arange(lines, dtype=np.int64)
    pos = np.arange(length, dtype=np.int64)
    j = js[line % len(js)]
    phase = 2.0 * math.pi * ((j[:, None] * pos[None, :]) % length) / length + 0.37 * line[:, None]
    f = torch.from_numpy(np.stack([np.cos(phase), np.sin(phase)])).float()          # [2, lines, length]
    return f.transpose(-1, -2).contiguous() if along_y else f


def impulse_pixels(h, w, pml=PML):
    """[(row, column, re, im)]: both PMLs, their inner edges, the four corners, the interior, and the lines that can start the last block of a
    pass (length - 2^m on either axis)."""
    ph, pw = min(pml, h // 2), min(pml, w // 2)
    px = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (ph // 2, w // 2 + 1), (h // 2 - 2, w - 1 - pw // 2), (ph - 1, pw), (h - ph, w - 1 - pw),
          (h // 2 + 1, w // 3)]
    px += [(h - s, w // 2) for s in (2, 4, 8, 16) if s < h] + [(h // 2, w - s) for s in (2, 4, 8, 16) if s < w]
    out, seen = [], set()
    for m, (y, x) in enumerate(px):
        if (y, x) in seen:
            continue
        seen.add((y, x))
        ang = 0.9 * m + 0.2
        out.append((y, x, (0.5 + 0.03 * m) * math.cos(ang), (0.5 + 0.03 * m) * math.sin(ang)))
    return out


def impulse_field(h, w, pml=PML):
    f = torch.zeros(2, h, w, dtype=torch.float32)
    for y, x, re, im in impulse_pixels(h, w, pml):
        f[0, y, x] = re
        f[1, y, x] = im
    return f


def noise_field(h, w, seed_offset=77):
    rng = np.random.default_rng(seed_offset + 4096 * h + w)
    f = torch.from_numpy((0.5 * rng.standard_normal((2, h, w))).astype(np.float32))
    return f / f.abs().max()


def probe_batch(h, w, pml=PML):
    """float32 [4, 2, h, w] in the order of PROBES."""
    return torch.stack([noise_field(h, w), mode_field(h, w), mode_field(h, w, along_y=True), impulse_field(h, w, pml)]).contiguous()


def seeded_k_sq(h, w, b, seed):
    g = torch.Generator().manual_seed(seed)
    sos = 1.0 + torch.rand(b, 1, h, w, generator=g, dtype=torch.float32)
    return ((1.0 / sos) ** 2).contiguous()


def seeded_src(h, w, b, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 2, h, w, generator=g, dtype=torch.float32)


_cases = {}


def forward_case(h, w, domain=DOMAIN):
    """SP.forward_case for (h, w): probes, k_sq, sources (one for the batch, one per sample), the float64 Laplacian / residuals and the bars."""
    key = (h, w, domain)
    if key not in _cases:
        t = tables(h, w, domain)
        u = probe_batch(h, w, domain[0])
        nb = u.shape[0]
        k_sq = seeded_k_sq(h, w, nb, 5000 + 3 * h + w)
        src1, srcb = seeded_src(h, w, 1, 6000 + 3 * h + w), seeded_src(h, w, nb, 7000 + 3 * h + w)
        lap = O.apply_laplacian(u.double(), t).contiguous()
        scale = float(lap[0].abs().max())                                   # sample 0 is the normalised noise
        ku = k_sq.double() * u.double()
        peak = SP.peak
        _cases[key] = dict(u=u, k_sq=k_sq, src1=src1, srcb=srcb, lap=lap, res1=lap + ku - src1.double(), resb=lap + ku - srcb.double(), scale=scale,
                           bar_lap=SP.BAR * scale * peak(u), bar_res1=SP.BAR * (scale * peak(u) + peak(ku) + float(src1.abs().max())),
                           bar_resb=SP.BAR * (scale * peak(u) + peak(ku) + peak(srcb)))
    return _cases[key]


# ---- seeded solver inputs ----------------------------------------------------------------------------------------------------------------------
def teacher_inputs(h, w, b, seed, depth=4):
    """golden_inputs.teacher_inputs for (h, w): white-noise wavefield / residual / hidden state and a random SoS in [1, 2]."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    return {
        "wf": torch.from_numpy((0.5 * rng.standard_normal((b, 2, h, w))).astype(f32)),
        "res": torch.from_numpy((5e-3 * rng.standard_normal((b, 2, h, w))).astype(f32)),
        "states": torch.from_numpy((0.5 * rng.standard_normal((b, 2, state_len(h, w, depth)))).astype(f32)),
        "sos": torch.from_numpy((1.0 + rng.random((b, 1, h, w))).astype(f32)),
    }


def point_source_map(h, w, location, amplitude):
    """O.point_source_map for (h, w) without smoothing: |ifft2(ifftshift(fftshift(fft2(delta * amp))))| as the real part -> [1, 2, h, w]."""
    m = torch.zeros((h, w))
    m[location[0], location[1]] = amplitude
    a = torch.abs(torch.fft.ifft2(torch.fft.ifftshift(torch.fft.fftshift(torch.fft.fft2(m)))))
    return torch.stack([a, torch.zeros_like(a)], 0).unsqueeze(0)


def box_sos(h, w, b):
    """sos = 1 with a 1.5 box, shifted per sample."""
    sos = torch.ones(b, 1, h, w)
    for s in range(b):
        y0, x0 = h // 3 + 2 * s, w // 3 + 3 * s
        sos[s, 0, y0:y0 + h // 4, x0:x0 + w // 4] = 1.5
    return sos


def oracle_loop(h, w, b, n_iter, weights, dtype, loc=None, amplitude=10.0):
    """n_iter iterations from rest on box_sos with a point source, in ``dtype``: (wavefield, [n_iter, b] RMSE trace)."""
    t = tables(h, w, DOMAIN, dtype)
    wd = {k: v.to(dtype) for k, v in weights.items()}
    loc = loc or [h // 4, w // 2]
    src = point_source_map(h, w, loc, amplitude).to(dtype)
    k_sq, wf = O.get_initials(box_sos(h, w, b).to(dtype), 1.0)
    states = [torch.zeros(b, 2, h >> d, w >> d, dtype=dtype) for d in range(4)]
    res = O.get_residual(wf, k_sq, src, t)
    trace = []
    with torch.no_grad():
        for _ in range(n_iter):
            wf, res, states = O.single_step(wf, k_sq, res, states, wd, src, t)
            trace.append(O.test_loss_function(res))
    return wf, torch.stack(trace)
