"""What test_spectral_mixed_host.py and test_spectral_mixed_gpu.py share, built on tests/spectral_probes.py: the same four probes, the same float64
reference (SP.forward_case, SP.adjoint_case) and the same bar (SP.BAR = 1e-5 of scale(n) * max|u|) -- the project's bar for every spectral route.

Added here for the mixed route (HN_OPT_SPECTRAL_MIXED, n = P * Q with a runtime odd P; k_spec_line of hn_spectral_line.hip):

  * a second pair of mode fields.  SP.mode_indices(n) adds the P / Q specific modes only where P is 3, 5 or 7, so these carry, one Fourier mode per
    line by SP.mode_field's own formula, the indices P, Q, Q -+ 1, 2 Q + P, n - Q, n - P, P * (Q / 2) and Q * ((P - 1) / 2): the modes whose
    Good-Thomas coordinates (k1, k2) are (0, .), (., 0), next to them, and the Nyquist lines of both factors.  Float64 Laplacian: SP.laplacian_ref.
  * a torch fp32 restatement of the kernels' algorithm (Good-Thomas gather, complex64 Q-point torch.fft, the P-point DFT as a complex64 matrix
    product, fp32 tables permuted by the output map, the inverse the same way): the CPU test shows with it that the bar is one a correct fp32
    kernel of this structure can meet, and that one wrong entry of the permuted k table fails it.
"""
import math

import numpy as np
import torch

import spectral_probes as SP
from helmnet_amd.laplacian import k_grid, pml_profile, spectral_route

# n -> why it is a GPU case (test_spectral_mixed_gpu.py); P * Q in the comment
GPU_SIZES = {
    144: "9 * 16: smallest n, smallest P and Q",
    176: "11 * 16: prime P",
    240: "15 * 16: P divisible by 3 and 5; must not go to the prime-factor kernels",
    288: "9 * 32: Q = 32 (odd log2 Q: the lone radix-2 stage)",
    400: "25 * 16",
    576: "9 * 64: Q = 64",
    1152: "9 * 128: largest Q",
    1040: "65 * 16: one sample per call (SP.ONE_AT_A_TIME)",
    2032: "127 * 16: largest P, largest line, largest LDS; batch 1",
}
EXTRA_NAMES = ("pq_modes_x", "pq_modes_y")


def legal_sizes():
    return list(range(SP.N_MIN, SP.N_MAX + 1, 16))


def factor(n):
    """(P, Q): n = P * Q, P odd, Q a power of two."""
    q = n & -n
    return n // q, q


def extra_mode_indices(n):
    p, q = factor(n)
    js = [p, q, q - 1, q + 1, 2 * q + p, n - q, n - p, p * (q // 2), q * ((p - 1) // 2)]
    out = []
    for j in js:
        if j % n not in out:
            out.append(j % n)
    return out


def extra_mode_field(n, along_y=False):
    """SP.mode_field's formula over extra_mode_indices(n)."""
    js = np.asarray(extra_mode_indices(n), dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    j = js[i % len(js)]
    phase = 2.0 * math.pi * ((j[:, None] * i[None, :]) % n) / n + 0.37 * i[:, None]
    f = torch.from_numpy(np.stack([np.cos(phase), np.sin(phase)])).float()
    return f.transpose(-1, -2).contiguous() if along_y else f


_extra = {}


def extra_case(n, domain=SP.DOMAIN):
    """The two extra mode fields with their float64 Laplacian and residual (k_sq and the broadcast source of SP.forward_case), computed once; the
    bars are SP.forward_case's formulas with its scale(n)."""
    key = (n, domain)
    if key not in _extra:
        for k in [k for k in _extra if k[0] >= SP.ONE_AT_A_TIME and k[0] != n]:
            del _extra[k]
        c = SP.forward_case(n, domain)
        u = torch.stack([extra_mode_field(n), extra_mode_field(n, along_y=True)]).contiguous()
        k_sq = c["k_sq"][1:3].contiguous()
        lap = SP.laplacian_ref(u, n, domain)
        ku = k_sq.double() * u.double()
        res1 = lap + ku - c["src1"].double()
        _extra[key] = dict(u=u, k_sq=k_sq, src1=c["src1"], lap=lap, res1=res1, bar_lap=SP.BAR * c["scale"] * SP.peak(u),
                           bar_res1=SP.BAR * (c["scale"] * SP.peak(u) + SP.peak(ku) + float(c["src1"].abs().max())))
    return _extra[key]


# ---- the algorithm in torch fp32 ----------------------------------------------------------------------------------------------------------------
def good_thomas(n):
    """(gather [P, Q]: natural index of (n1, n2); kmap [P, Q]: natural frequency of (k1, k2)) of n = P * Q."""
    p, q = factor(n)
    qinv = next(x for x in range(1, p + 1) if (q * x) % p == 1)
    pinv = next(x for x in range(1, q + 1) if (p * x) % q == 1)
    n1, n2 = np.arange(p)[:, None], np.arange(q)[None, :]
    return (q * n1 + p * n2) % n, (q * qinv * n1 + p * pinv * n2) % n


def restated_tables(n, domain=SP.DOMAIN):
    """fp32 tables as spec_build makes them: float64, then cast; -k^2 squared in fp32; the k tables permuted by the output map."""
    pml, sigma_max, k = domain
    p, q = factor(n)
    gather, kmap = good_thomas(n)
    k32 = torch.from_numpy(k_grid(n)).float()
    _, a, b = pml_profile(n, pml, sigma_max, k)
    m = np.arange(p)
    wp = torch.from_numpy(np.exp(-2j * np.pi * ((m[:, None] * m[None, :]) % p) / p)).to(torch.complex64)
    return dict(p=p, q=q, gather=torch.from_numpy(gather.reshape(-1)), k1p=k32[torch.from_numpy(kmap)].clone(),
                k2p=(-(k32 * k32))[torch.from_numpy(kmap)].clone(), a=torch.from_numpy(a).to(torch.complex64),
                b=torch.from_numpy(b).to(torch.complex64), wp=wp)


def _restated_axis(x, t):
    """a * D1 x + b * D2 x along the last axis of the complex64 x."""
    p, q = t["p"], t["q"]
    n = p * q
    g = x[..., t["gather"]].reshape(x.shape[:-1] + (p, q))
    spec = torch.fft.fft(g, dim=-1)                                  # P interleaved Q-point transforms
    spec = torch.matmul(t["wp"], spec)                               # P-point DFT across them
    d1 = torch.complex(-spec.imag * t["k1p"], spec.real * t["k1p"])  # (0, k) * U
    d2 = spec * t["k2p"]
    out = []
    for d in (d1, d2):
        d = torch.matmul(t["wp"].conj(), d)
        d = torch.fft.ifft(d, dim=-1) * q                            # unnormalised, as the kernels run it
        nat = torch.empty_like(x)
        nat[..., t["gather"]] = d.reshape(x.shape)
        out.append(nat / n)
    return t["a"] * out[0] + t["b"] * out[1]


def restated_laplacian(u, n, domain=SP.DOMAIN, tables=None):
    """fp32 [B, 2, n, n] -> fp32 Laplacian by the algorithm of the mixed kernels."""
    t = tables or restated_tables(n, domain)
    x = torch.complex(u[:, 0], u[:, 1])
    out = _restated_axis(x, t) + _restated_axis(x.transpose(-1, -2), t).transpose(-1, -2)
    return torch.stack([out.real, out.imag], 1).contiguous()


def mutate_k1p_entry(t, j):
    """The entry of the permuted k table that frequency j reads swaps values with its neighbour along k2."""
    _, kmap = good_thomas(t["p"] * t["q"])
    a1, a2 = (int(v[0]) for v in np.nonzero(kmap == j))
    nb = a2 + 1 if a2 + 1 < t["q"] else a2 - 1
    k1p = t["k1p"].clone()
    k1p[a1, a2], k1p[a1, nb] = t["k1p"][a1, nb], t["k1p"][a1, a2]
    return dict(t, k1p=k1p)


def mixed_lines(n, nbuf, batch):
    """Lines per block on the mixed route: rect_lines(n, n, nbuf, batch) of hn_spectral_line.hip, the one rule of every LDS-line launch; nbuf = 4
    forward, 3 adjoint."""
    lines = 16
    while lines > 1 and lines * nbuf * n * 8 > 80 * 1024:
        lines //= 2
    while lines > 1 and ((n + lines - 1) // lines) * batch < 512:
        lines //= 2
    return lines

