"""Probes, float64 references and the error bar shared by test_spectral_host.py and test_spectral_gpu.py.

Reference: the CPU oracle on float64 tensors with float64 tables (``O.SpectralTables(..., dtype=torch.float64)`` with ``O.apply_laplacian`` /
``O.get_residual``; the adjoint is ``torch.autograd.grad`` through the float64 ``O.get_residual``).  Every input is fp32-representable and up-cast.

Bar: the project's "1e-5 * max"  at the OPERATOR's scale, not each probe's:
    scale(n) = max |L64(w)|,  w = the seeded noise of teacher_inputs(n, 1, seed=77 + n)["wf"] divided by its own max-abs   (7.3 .. 7.6 for n >= 256)
    a probe u passes when  max |got - want| <= 1e-5 * (scale(n) * max|u| + max|k_sq * u| + max|src|)       (the last two for the residual only)
A low-frequency mode has an output of about 1e-3 * max|u|: fp32 arithmetic on inputs of size 1 cannot be right to 1e-5 of THAT, and the fp32
reference is not either.

Probes (samples of one batch where n < 1024, one at a time above that -- a float64 application at n = 2048 takes about a second):
    noise     w above: every frequency at once; blind to a single wrong table entry at large n (its share of the output is ~1 / n)
    modes_x   line i carries exp(i (2 pi j_i x / n + 0.37 i)), j_i cycling through mode_indices(n): one frequency-table entry per line, so a wrong
              k entry, twiddle or Good-Thomas index shows at full size on that line
    modes_y   the same, transposed
    impulses  single pixels with different complex values: in the PML, on its inner edge, at (0, 0) and (n - 1, n - 1), in the interior, and on
              every line that can start the last block of a pass (n - 2^m; the last 256-wide block of the dense kernel)
"""
import math

import numpy as np
import torch

from golden_inputs import teacher_inputs
from oracle import helmnet_oracle as O

PML, SIGMA_MAX, K = 8, 2.0, 1.0
DOMAIN = (PML, SIGMA_MAX, K)
BAR = 1e-5
PROBES = ("noise", "modes_x", "modes_y", "impulses")
ONE_AT_A_TIME = 1024          # from this size on the reference (and the GPU call) handles one sample per call
N_MIN, N_MAX = 16, 2048       # hn_set_domain's limits (include/helmnet_hip.h); n must be a multiple of 16

DENSE_SIZES = (144, 176, 208, 272, 1040)     # 1040: the last k_spec_dense block of a line has 16 live threads


def pow2_sizes():
    return [n for n in range(N_MIN, N_MAX + 1) if n & (n - 1) == 0]


def pfa_pairs():
    """(P, Q) of every size the rule of include/helmnet_hip.h (HN_OPT_SPECTRAL_PFA: n = 3 * 2^k, 5 * 2^k, 7 * 2^k) leaves inside hn_set_domain's
    limits (a multiple of 16 in [16, 2048])."""
    out = []
    for p in (3, 5, 7):
        q = 1
        while p * q <= N_MAX:
            if (p * q) % 16 == 0 and p * q >= N_MIN:
                out.append((p, q))
            q *= 2
    return out


def pfa_factor(n):
    for p, q in pfa_pairs():
        if p * q == n:
            return p, q
    return None


def pfa_sizes():
    return [p * q for p, q in pfa_pairs()]


def forward_sizes():
    return pow2_sizes() + pfa_sizes() + list(DENSE_SIZES)


def route(n):
    return "radix-4" if n & (n - 1) == 0 else "pfa" if pfa_factor(n) else "dense"


def mode_indices(n):
    js = [0, 1, 2, 3, 5, 7, 16, n // 16, n // 8 - 1, n // 4 + 1, n // 3, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1]
    pq = pfa_factor(n)
    if pq:
        p, q = pq
        js += [p, q, q - 1, q + 1, 2 * q + p, n - q]
    out = []
    for j in js:
        if j % n not in out:
            out.append(j % n)
    return out


def mode_field(n, along_y=False):
    js = np.asarray(mode_indices(n), dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    j = js[i % len(js)]
    phase = 2.0 * math.pi * ((j[:, None] * i[None, :]) % n) / n + 0.37 * i[:, None]
    f = torch.from_numpy(np.stack([np.cos(phase), np.sin(phase)])).float()
    return f.transpose(-1, -2).contiguous() if along_y else f


def impulse_pixels(n, pml=PML):
    """[(row, column, re, im)]: the lines named in the module docstring, every pixel with its own complex value."""
    pml = min(pml, n // 2)
    px = [(0, 0), (n - 1, n - 1), (pml // 2, n // 2 + 1), (n // 2 - 2, n - 1 - pml // 2), (pml - 1, pml), (n - pml, n - 1 - pml), (n // 2 + 1, n // 3)]
    px += [(n - s, n - s) for s in (2, 4, 8, 16, 32, 64) if s < n]
    x_last = 256 * ((n - 1) // 256)
    px += [(n // 4, x_last), (x_last, n // 4 + 1)]
    out, seen = [], set()
    for m, (y, x) in enumerate(px):
        if (y, x) in seen:
            continue
        seen.add((y, x))
        ang = 0.9 * m + 0.2
        out.append((y, x, (0.5 + 0.03 * m) * math.cos(ang), (0.5 + 0.03 * m) * math.sin(ang)))
    return out


def impulse_field(n, pml=PML):
    f = torch.zeros(2, n, n, dtype=torch.float32)
    for y, x, re, im in impulse_pixels(n, pml):
        f[0, y, x] = re
        f[1, y, x] = im
    return f


def noise_field(n, seed_offset=77):
    w = torch.from_numpy(teacher_inputs(n, 1, seed=seed_offset + n)["wf"][0])
    return w / w.abs().max()


def probe_batch(n, pml=PML):
    """float32 [4, 2, n, n] in the order of PROBES."""
    return torch.stack([noise_field(n), mode_field(n), mode_field(n, along_y=True), impulse_field(n, pml)]).contiguous()


# ---- float64 reference --------------------------------------------------------------------------------------------------------------------------
_tables, _cases = {}, {}


def _evict(cache, n):
    """The float64 tables and fields of a size >= 1024 take hundreds of MB: keep those of one such size at a time."""
    if n >= ONE_AT_A_TIME:
        for key in [k for k in cache if k[0] >= ONE_AT_A_TIME and k[0] != n]:
            del cache[key]


def tables(n, domain=DOMAIN, dtype=torch.float64):
    key = (n, domain, dtype)
    if key not in _tables:
        _evict(_tables, n)
        _tables[key] = O.SpectralTables(n, *domain, dtype=dtype)
    return _tables[key]


def apply_each(fn, n, *fields):
    """fn on the whole batch where n < ONE_AT_A_TIME, else sample by sample (fields of batch 1 are passed as they are)."""
    b = fields[0].shape[0]
    if n < ONE_AT_A_TIME or b == 1:
        return fn(*fields)
    return torch.cat([fn(*(f if f.shape[0] == 1 else f[s:s + 1] for f in fields)) for s in range(b)])


def laplacian_ref(u, n, domain=DOMAIN, dtype=torch.float64, t=None):
    t = t or tables(n, domain, dtype)
    return apply_each(lambda x: O.apply_laplacian(x.to(dtype), t).contiguous(), n, u)


def adjoint_ref(g, k_sq, n, domain=DOMAIN):
    """J^T g of the float64 O.get_residual with respect to the wavefield (the residual is linear in it: any base point)."""
    t = tables(n, domain)
    one_graph = n >= ONE_AT_A_TIME            # then every cotangent has the same k_sq (adjoint_case): one forward pass serves them all
    assert not one_graph or all(torch.equal(k_sq[s], k_sq[0]) for s in range(k_sq.shape[0]))
    wf = torch.zeros((1,) + g.shape[1:] if one_graph else g.shape, dtype=torch.float64, requires_grad=True)
    res = O.get_residual(wf, (k_sq[:1] if one_graph else k_sq).double(), torch.zeros(1, 2, n, n, dtype=torch.float64), t)
    if not one_graph:
        return torch.autograd.grad(res, wf, g.double())[0]
    return torch.cat([torch.autograd.grad(res, wf, g[s:s + 1].double(), retain_graph=True)[0] for s in range(g.shape[0])])


def seeded_k_sq(n, b, seed):
    g = torch.Generator().manual_seed(seed)
    sos = 1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float32)
    return ((1.0 / sos) ** 2).contiguous()


def seeded_src(n, b, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, 2, n, n, generator=g, dtype=torch.float32)


def peak(x):
    """max |x| of every sample -> [B] float64."""
    return x.double().abs().flatten(1).max(1).values


def forward_case(n, domain=DOMAIN):
    """Probes, k_sq, sources and the float64 Laplacian / residual of one size and domain, computed once."""
    key = (n, domain, "fwd")
    if key not in _cases:
        _evict(_cases, n)
        u = probe_batch(n, domain[0])
        k_sq = seeded_k_sq(n, len(PROBES), 5000 + n)
        src1, src2 = seeded_src(n, 1, 6000 + n), seeded_src(n, 2, 7000 + n)
        lap = laplacian_ref(u, n, domain)
        scale = float(lap[0].abs().max())                                   # sample 0 is w
        ku = k_sq.double() * u.double()
        res1 = lap + ku - src1.double()
        res2 = lap[:2] + ku[:2] - src2.double()
        bar_lap = BAR * scale * peak(u)
        bar_res1 = BAR * (scale * peak(u) + peak(ku) + float(src1.abs().max()))
        bar_res2 = BAR * (scale * peak(u[:2]) + peak(ku[:2]) + peak(src2))
        _cases[key] = dict(u=u, k_sq=k_sq, src1=src1, src2=src2, lap=lap, res1=res1, res2=res2, scale=scale,
                           bar_lap=bar_lap, bar_res1=bar_res1, bar_res2=bar_res2)
    return _cases[key]


ADJOINT_PROBES = 3        # noise and the two mode fields as cotangents


def adjoint_case(n, domain=DOMAIN):
    """Cotangents (the noise and mode probes), k_sq and the float64 L^H g + k_sq g; the scale is max |L^H64(w)| of the same noise w."""
    key = (n, domain, "adj")
    if key not in _cases:
        _evict(_cases, n)
        g = probe_batch(n, domain[0])[:ADJOINT_PROBES].contiguous()
        k_sq = seeded_k_sq(n, len(PROBES), 5000 + n)[:ADJOINT_PROBES].contiguous()
        if n >= ONE_AT_A_TIME:                                               # one at a time: one k_sq map serves every cotangent
            k_sq = k_sq[:1].repeat(ADJOINT_PROBES, 1, 1, 1)
        vjp = adjoint_ref(g, k_sq, n, domain)
        kg = k_sq.double() * g.double()
        scale = float((vjp[0] - kg[0]).abs().max())
        # the other field of the inner-product identity <L u, g> = <u, L^H g>: a second noise plus the (normalised) expected L^H g itself.  Against
        # plain noise the product of a mode field nearly cancels (1.4 at n = 128, a sum of 3e4 terms of size 1), and 1e-5 of THAT is below the
        # rounding of the sum; with a part along L^H g both sides are about |L^H g|^2 / scale
        u = (0.5 * noise_field(n, seed_offset=78)[None] + (vjp / scale).float()).contiguous()
        _cases[key] = dict(g=g, k_sq=k_sq, vjp=vjp, scale=scale, bar=BAR * (scale * peak(g) + peak(kg)), u=u)
    return _cases[key]


def errors(got, want):
    """max |got - want| of every sample -> [B] float64 (got: fp32 from the GPU or the fp32 oracle)."""
    return peak(got.detach().cpu().double() - want)


def mutate_k_entry(t, j=5):
    """The mutant the mode probes exist for: entry j of the x wavenumber tables (i k and -k^2) takes its neighbour's value."""
    for tab in (t.kx, t.kx_sq):
        tab[:, :, j, :] = tab[:, :, j - 1, :]
    return t
