"""The probes and the bar of tests/spectral_probes.py, checked on the CPU (no GPU needed):

  * the fp32 oracle -- an fp32 implementation of the operator nobody doubts -- meets the bar on every probe with a factor 4 to spare, so the bar
    is one a correct fp32 kernel can meet (measured here: <= 1.4e-6 of scale * max|u| against 1e-5);
  * a mutant with ONE wrong wavenumber-table entry fails the mode probe at n = 768 while the noise probe stays under the bar: the reason the
    mode probes exist;
  * the size lists of test_spectral_gpu.py contain every kernel instance hn_spectral.hip dispatches to, derived from the header's rule.
"""
import copy
import os
import re

import pytest
import torch

import spectral_probes as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [48, 256, 768])
def test_fp32_oracle_meets_the_bar_with_a_factor_four_to_spare(n):
    c = SP.forward_case(n)
    u = c["u"]
    t32 = SP.tables(n, dtype=torch.float32)
    lap32 = SP.laplacian_ref(u, n, dtype=torch.float32, t=t32)
    res32 = lap32 + c["k_sq"] * u - c["src1"]
    assert lap32.dtype == torch.float32 and c["lap"].dtype == torch.float64
    e_lap, e_res = SP.errors(lap32, c["lap"]), SP.errors(res32, c["res1"])
    for i, name in enumerate(SP.PROBES):
        print(f"n={n} {name}: fp32 oracle laplacian {float(e_lap[i] / c['bar_lap'][i]) * SP.BAR:.2e}, residual "
              f"{float(e_res[i] / c['bar_res1'][i]) * SP.BAR:.2e} of the scale (bar {SP.BAR:.0e}); scale(n) = {c['scale']:.3f}")
    assert bool((4 * e_lap <= c["bar_lap"]).all()), (e_lap / c["bar_lap"]).tolist()
    assert bool((4 * e_res <= c["bar_res1"]).all()), (e_res / c["bar_res1"]).tolist()
    a = SP.adjoint_case(n)
    g = a["g"].clone().requires_grad_(True)
    # the fp32 adjoint: autograd through the fp32 oracle
    from oracle import helmnet_oracle as O
    res = O.get_residual(g, a["k_sq"], torch.zeros(1, 2, n, n), t32)
    (vjp32,) = torch.autograd.grad(res, g, a["g"])
    e_adj = SP.errors(vjp32, a["vjp"])
    print(f"n={n}: fp32 oracle adjoint {[f'{float(x) * SP.BAR:.2e}' for x in e_adj / a['bar']]} of the scale; adjoint scale {a['scale']:.3f}")
    assert bool((4 * e_adj <= a["bar"]).all()), (e_adj / a["bar"]).tolist()


def test_one_wrong_k_entry_is_caught_by_the_modes_and_missed_by_the_noise():
    n = 768
    c = SP.forward_case(n)
    mutant = SP.mutate_k_entry(copy.deepcopy(SP.tables(n)), j=5)
    assert 5 in SP.mode_indices(n)
    got = SP.laplacian_ref(c["u"], n, t=mutant)
    frac = SP.errors(got, c["lap"]) / (c["scale"] * SP.peak(c["u"]))
    print(f"n={n}, k table entry 5 := entry 4: error / (scale * max|u|) = " + ", ".join(f"{p} {float(f):.2e}" for p, f in zip(SP.PROBES, frac)))
    noise, modes_x = float(frac[0]), float(frac[1])
    assert 0.0 < noise <= SP.BAR           # white noise in max-norm: under the bar -- the existing kind of test passes the mutant
    assert modes_x > 10 * SP.BAR           # one mode per line: the lines that carry mode 5 are wrong at full size


def test_probes_are_what_the_docstring_says():
    for n in (16, 48, 1040):
        u = SP.probe_batch(n)
        assert u.dtype == torch.float32 and u.shape == (4, 2, n, n)
        assert float(u[0].abs().max()) == 1.0
        # every line of modes_x is a single Fourier mode of unit modulus; modes_y is its transpose
        spec = torch.fft.fft(torch.complex(u[1, 0], u[1, 1]).to(torch.complex128), dim=-1).abs() / n
        js = SP.mode_indices(n)
        for i in range(n):
            j = js[i % len(js)]
            assert abs(float(spec[i, j]) - 1.0) < 1e-6 and float(spec[i].sum() - spec[i, j]) < 1e-4, (n, i, j)
        assert torch.equal(u[2], u[1].transpose(-1, -2))
        px = SP.impulse_pixels(n)
        assert int((u[3].abs().sum(0) > 0).sum()) == len(px) and len({(round(r, 6), round(i, 6)) for _, _, r, i in px}) == len(px)
        assert {(0, 0), (n - 1, n - 1)} <= {(y, x) for y, x, _, _ in px}
    assert {3, 32, 31, 33, 67, 64} <= set(SP.mode_indices(96))        # P, Q, Q -+ 1, 2 Q + P, n - Q


def test_the_gpu_parametrisation_covers_every_kernel_instance():
    """Every power of two and every P * Q the header's rule allows is a forward AND an adjoint case of test_spectral_gpu.py, and the set built from
    the rule is the set of instances hn_spectral.hip dispatches to (its HN_PFA lists and power-of-two cases)."""
    import test_spectral_gpu as G
    src = open(os.path.join(REPO, "helmnet_amd", "csrc", "hn_spectral.hip")).read()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    assert "n = 3 * 2^k, 5 * 2^k, 7 * 2^k" in hdr                       # the rule pfa_pairs() restates
    pow2 = {n for n in range(16, 2049, 16) if n & (n - 1) == 0}
    pfa = {p * 2 ** k for p in (3, 5, 7) for k in range(12) if 16 <= p * 2 ** k <= 2048 and (p * 2 ** k) % 16 == 0}
    assert set(SP.pow2_sizes()) == pow2 and len(pow2) == 8
    assert set(SP.pfa_sizes()) == pfa and len(pfa) == 16
    for sizes in (G.FORWARD_SIZES, G.ADJOINT_SIZES):
        assert pow2 <= set(sizes) and pfa <= set(sizes) and set(SP.DENSE_SIZES) <= set(sizes)
        assert len(sizes) == len(set(sizes))
    # the kernel instances in the source: HN_PFA(Q, P) of the forward and of the adjoint dispatch, and their power-of-two cases
    fwd, adj = src.split("int spec_apply(")[1].split("int spec_adjoint(")[0], src.split("int spec_adjoint(")[1]
    for body in (fwd, adj):
        inst = {(int(p), int(q)) for q, p in re.findall(r"HN_PFA\((\d+), (\d+)\)", body)}
        assert inst == set(SP.pfa_pairs()), inst ^ set(SP.pfa_pairs())
    assert {int(x) for x in re.findall(r"case (\d+):", fwd)} == pow2
    assert {int(x) for x in re.findall(r"HN_ADJ\((\d+)\)", adj)} == pow2
    for n in SP.forward_sizes():
        assert SP.route(n) == ("radix-4" if n in pow2 else "pfa" if n in pfa else "dense")
    # the option cases: all nine 256 combinations, both 512 routes, the dense operator at PFA-able sizes, the launch shapes that depend on the batch
    assert sorted(G.OPTIONS_256) == [(r, c) for r in range(3) for c in range(3)] and G.OPTIONS_512 == [0, 1]
    assert all(SP.route(n) == "pfa" for n in G.PFA_OFF_SIZES)
    assert G.BATCH_SHAPES == {768: (1, 2, 3), 1280: (1, 2), 1792: (1,)}
    for n, batches in G.BATCH_SHAPES.items():
        shapes = [G.pfa_launch_shape(n, b) for b in batches]
        assert len({lpb for lpb, _ in shapes}) == len(batches) or n == 1792, shapes      # a different lines-per-block for every batch listed
    assert [G.pfa_launch_shape(768, b)[0] for b in (1, 2, 3)] == [1, 2, 4]
    assert G.pfa_launch_shape(1792, 1)[1] > 48 * 1024 and G.pfa_launch_shape(1280, 2)[1] > 48 * 1024 >= G.pfa_launch_shape(1280, 1)[1]
    assert max(G.pfa_launch_shape(n, b)[1] for n in SP.pfa_sizes() for b in (1, 2, 3, 4, 512)) <= 96 * 1024   # the attribute the launch sets
