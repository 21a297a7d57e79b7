"""The FFT route of the float64 operator (HN_OPT_F64_FFT, hn_f64_fft.hip) on the CPU; no GPU needed.

  * the header's enums and the ctypes tables carry the new option and counter with the same, unique values;
  * helmnet_amd.laplacian.f64_route, the context-free twin of the routing rule, over all 128 legal sizes against the factor rule restated here;
  * a numpy float64 model of ONE line's algorithm as the kernel runs it -- Good-Thomas slot map, in-place Q-point transforms that leave the spectrum
    bit-reversed, a direct P-point DFT across them, the derivative multipliers in the order the spectrum is met, the inverses, 1 / n at the end --
    against the oracle's apply_laplacian on float64 tables.  Bar 1e-12 * max|expected|: both sides are O(log n) deep float64 transforms of O(1) data
    (rounding ~ 1e-15 relative to the largest term), which leaves a factor of a few hundred.  This pins the table conventions the kernel's host code
    follows (build_tables): slot[i] = n1 Q + n2 with i = (Q n1 + P n2) mod n, and position (a1, r) holding frequency (Q qinv a1 + P pinv bitrev(r)) mod n;
  * the dynamic LDS of every legal size, by the kernel's arithmetic restated here, fits what one workgroup may declare (160 KiB)."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PML, SIGMA_MAX, K = 8, 2.0, 1.0
SIZES = list(range(16, 2049, 16))


def factor(n):
    """n = P * Q with Q the largest power of two that divides n."""
    q = 1
    while n % (2 * q) == 0:
        q *= 2
    return n // q, q


def test_header_and_binding_tables_carry_the_option_and_the_counter():
    from helmnet_amd import _lib
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    pairs = re.findall(r"\b(HN_[A-Z0-9_]+)\s*=\s*(-?\d+)", hdr)
    enums = {name: int(val) for name, val in pairs}
    assert enums["HN_OPT_F64_FFT"] == _lib.HN_OPTION["f64_fft"] == 18 < 100
    assert enums["HN_CNT_F64_ROUTE"] == _lib.HN_COUNTER["f64_route"] == 8
    assert list(_lib.HN_OPTION.values()).count(18) == 1 and list(_lib.HN_COUNTER.values()).count(8) == 1
    assert [v for k, v in enums.items() if k.startswith(("HN_OPT_", "HN_EXP_"))].count(18) == 1
    assert [v for k, v in enums.items() if k.startswith("HN_CNT_")].count(8) == 1
    assert "#define HN_ABI_VERSION 7" in hdr            # a new option and a new counter, no new symbol
    assert "hn_f64_fft.hip" in open(os.path.join(REPO, "helmnet_amd", "build.py")).read()


def test_f64_route_follows_the_factor_rule_at_every_legal_size():
    from helmnet_amd.laplacian import f64_route
    assert len(SIZES) == 128
    for n in SIZES:
        p, q = factor(n)
        assert p * q == n and p % 2 == 1 and q & (q - 1) == 0
        assert 1 <= p <= 127 and 16 <= q <= 2048, (n, p, q)
        assert f64_route(n, 1) == ("fft", p, q)
        assert f64_route(n, 0) == f64_route(n) == ("dense",)
    for bad in (0, 8, 24, 2064):
        with pytest.raises(ValueError):
            f64_route(bad, 1)
    with pytest.raises(ValueError):
        f64_route(64, 2)


# ---- the line algorithm, restated ----
def bitrev(r, bits):
    return int(format(r, f"0{bits}b")[::-1], 2) if bits else 0


def line_tables(n, t64):
    p, q = factor(n)
    logq = q.bit_length() - 1
    qinv = pow(q, -1, p) if p > 1 else 0
    pinv = pow(p, -1, q)
    i = np.arange(n)
    slot = ((i % p) * qinv % p) * q + (i % q) * pinv % q                       # Good-Thomas input map: i = (Q n1 + P n2) mod n
    assert sorted(slot) == list(range(n))
    n1, n2 = slot // q, slot % q
    assert np.array_equal((q * n1 + p * n2) % n, i)
    freq = np.array([[(q * qinv * a1 + p * pinv * bitrev(r, logq)) % n for r in range(q)] for a1 in range(p)])   # output map, k2 bit-reversed
    assert sorted(freq.reshape(-1)) == list(range(n))
    k1 = t64.kx[0, 0, :, 1].numpy()                                            # the fp32 grid, up-cast; Nyquist at -pi
    k2 = t64.kx_sq[0, 0, :, 0].numpy()                                         # its fp32 square, negated, up-cast
    assert k1.dtype == np.float64 and k1[n // 2] == np.float64(np.float32(-np.pi)) and np.array_equal(k2, -(k1.astype(np.float32) ** 2).astype(np.float64))
    a = t64.ax[0, 0, :, 0].numpy() + 1j * t64.ax[0, 0, :, 1].numpy()
    b = t64.bx[0, 0, :, 0].numpy() + 1j * t64.bx[0, 0, :, 1].numpy()
    m = np.arange(p)
    return dict(p=p, q=q, logq=logq, slot=slot, k1m=k1[freq], k2m=k2[freq], a=a, b=b, twq=np.exp(-2j * np.pi * np.arange(q) / q),
                wp=np.exp(-2j * np.pi * (np.outer(m, m) % p) / p))


def fft_dif(x, t):
    """In place along the last axis (length Q): decimation in frequency, natural in, bit-reversed out."""
    q = t["q"]
    x = x.copy()
    span = q
    while span >= 2:
        v = x.reshape(x.shape[:-1] + (q // span, 2, span // 2))
        top, bot = v[..., 0, :].copy(), v[..., 1, :].copy()
        w = t["twq"][np.arange(span // 2) * (q // span)]
        v[..., 0, :] = top + bot
        v[..., 1, :] = (top - bot) * w
        span //= 2
    return x


def ifft_dit(x, t):
    """The transposed flow graph with conjugate twiddles: bit-reversed in, natural out, unnormalised."""
    q = t["q"]
    x = x.copy()
    span = 2
    while span <= q:
        v = x.reshape(x.shape[:-1] + (q // span, 2, span // 2))
        w = np.conj(t["twq"][np.arange(span // 2) * (q // span)])
        top, bot = v[..., 0, :].copy(), v[..., 1, :] * w
        v[..., 0, :] = top + bot
        v[..., 1, :] = top - bot
        span *= 2
    return x


def line_operator(x, t):
    """a . D1 x + b . D2 x along the last axis of the complex128 x, by the kernel's steps."""
    p, q = t["p"], t["q"]
    n = p * q
    buf = np.empty_like(x)
    buf[..., t["slot"]] = x                                             # 1: load through the slot map
    spec = fft_dif(buf.reshape(x.shape[:-1] + (p, q)), t)               # 2: P in-place Q-point transforms
    if p > 1:
        spec = np.einsum("ks,...sr->...kr", t["wp"], spec)              # 3: direct P-point DFT across them
    d1 = 1j * t["k1m"] * spec                                           #    (0, k) * U and (-k^2, 0) * U where the spectrum sits
    d2 = t["k2m"] * spec
    out = []
    for d in (d1, d2):
        if p > 1:
            d = np.einsum("ks,...sr->...kr", np.conj(t["wp"]), d)       # 4: inverse P-point DFT
        d = ifft_dit(d, t).reshape(x.shape)                             # 5: inverse Q-point transforms
        out.append(d[..., t["slot"]] / n)                               # 6: read back through the slot map, 1 / n
    return t["a"] * out[0] + t["b"] * out[1]


def test_bit_reversed_transform_pair_is_a_dft_and_its_inverse():
    rng = np.random.default_rng(3)
    for q in (16, 32, 128):
        t = dict(q=q, twq=np.exp(-2j * np.pi * np.arange(q) / q))
        x = rng.standard_normal((3, q)) + 1j * rng.standard_normal((3, q))
        logq = q.bit_length() - 1
        rev = np.array([bitrev(r, logq) for r in range(q)])
        assert np.abs(fft_dif(x, t) - np.fft.fft(x, axis=-1)[:, rev]).max() <= 1e-13 * q
        assert np.abs(ifft_dit(fft_dif(x, t), t) / q - x).max() <= 1e-14 * q


@pytest.mark.parametrize("n", [16, 48, 176, 272])
def test_line_algorithm_model_matches_the_float64_reference(n):
    t64 = O.SpectralTables(n, PML, SIGMA_MAX, K, dtype=torch.float64)
    t = line_tables(n, t64)
    g = torch.Generator().manual_seed(77 + n)
    wf = torch.randn(2, 2, n, n, generator=g, dtype=torch.float32).double()
    want = O.apply_laplacian(wf, t64).contiguous().numpy()
    x = wf[:, 0].numpy() + 1j * wf[:, 1].numpy()
    got = line_operator(x, t) + np.swapaxes(line_operator(np.swapaxes(x, -1, -2).copy(), t), -1, -2)   # row pass + column pass
    err = max(np.abs(got.real - want[:, 0]).max(), np.abs(got.imag - want[:, 1]).max())
    scale = np.abs(want).max()
    print(f"n={n} = {t['p']} * {t['q']}: line model vs reference {err / scale:.3e} of max|expected|")
    assert err <= 1e-12 * scale, (err, scale)


def test_every_legal_line_fits_one_workgroups_lds():
    """(3 or 4 buffers of n double2) + Q + P twiddles, one line per block; the issue's three worst cases by arithmetic."""
    need = {}
    for n in SIZES:
        p, q = factor(n)
        need[n] = ((3 if p == 1 else 4) * n + q + p) * 16
    assert need[2048] == 3 * 32 * 1024 + (2048 + 1) * 16 and need[2032] == 4 * 2032 * 16 + (16 + 127) * 16 and need[1536] == 96 * 1024 + (512 + 3) * 16
    assert max(need.values()) == need[2032] <= 160 * 1024
