"""The mixed spectral route (HN_OPT_SPECTRAL_MIXED: n = P * 2^k with a runtime odd P) on the CPU; no GPU needed.

  * helmnet_amd.laplacian.spectral_route, the Python twin of spec_build's rule, partitions the 128 legal sizes 8 / 16 / 104;
  * the ctypes tables carry the new option and counter with the header's values;
  * a torch fp32 restatement of the kernels' algorithm (tests/spectral_mixed_probes.py) meets the project's bar with a factor 3 to spare on the
    four probes and the two extra mode fields, so the bar is one a correct fp32 kernel of this structure can meet.  Measured error / bar:
    144 0.036, 400 0.065, 1040 0.138, 2032 0.293 (the P-point sums grow with P);
  * a mutant with ONE entry of the permuted k table swapped with its neighbour exceeds ten times the bar on the extra mode fields at n = 400.
"""
import os
import re

import pytest
import torch

import spectral_mixed_probes as MP
import spectral_probes as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spectral_route_partitions_the_legal_sizes():
    sizes = MP.legal_sizes()
    assert len(sizes) == 128
    on = {n: MP.spectral_route(n, mixed=1) for n in sizes}
    off = {n: MP.spectral_route(n) for n in sizes}
    count = lambda routes, name: sum(1 for r in routes.values() if r[0] == name)
    assert [count(on, k) for k in ("pow2", "prime_factor", "mixed", "dense")] == [8, 16, 104, 0]
    assert [count(off, k) for k in ("pow2", "prime_factor", "mixed", "dense")] == [8, 16, 0, 104]
    assert {n for n in sizes if on[n][0] == "pow2"} == set(SP.pow2_sizes())
    assert {n for n in sizes if on[n][0] == "prime_factor"} == set(SP.pfa_sizes())
    for n in sizes:
        name, p, q = on[n]
        assert p * q == n and p % 2 == 1 and q & (q - 1) == 0 and (p, q) == MP.factor(n)
        assert off[n][1:] == (p, q)
        if name == "mixed":
            assert 9 <= p <= 127 and q in (16, 32, 64, 128), (n, p, q)
            assert SP.route(n) == "dense"
    # without the prime-factor kernels their sixteen sizes are mixed too (P = 3, 5, 7 are odd factors like any other); without both: dense
    for n in SP.pfa_sizes():
        assert MP.spectral_route(n, pfa=0, mixed=1) == ("mixed",) + SP.pfa_factor(n)
        assert MP.spectral_route(n, pfa=0, mixed=0)[0] == "dense"
    assert all(MP.spectral_route(n, pfa=0, mixed=1)[0] == "pow2" for n in SP.pow2_sizes())
    assert set(MP.GPU_SIZES) <= {n for n in sizes if on[n][0] == "mixed"}
    with pytest.raises(ValueError):
        MP.spectral_route(2064)


def test_binding_tables_carry_the_option_and_the_counter():
    from helmnet_amd import _lib
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    enums = {name: int(val) for name, val in re.findall(r"\b(HN_[A-Z0-9_]+)\s*=\s*(-?\d+)", hdr)}
    assert _lib.HN_OPTION["spectral_mixed"] == enums["HN_OPT_SPECTRAL_MIXED"] < 100
    assert _lib.HN_COUNTER["spectral_route"] == enums["HN_CNT_SPECTRAL_ROUTE"]
    assert list(_lib.HN_OPTION.values()).count(_lib.HN_OPTION["spectral_mixed"]) == 1
    assert "n = P * 2^k, P odd >= 9" in hdr
    from helmnet_amd import build
    assert "hn_spectral_line.hip" in build.SOURCES
    assert "hn_spectral_mixed.hip" not in build.SOURCES and "hn_spectral_rect.hip" not in build.SOURCES
    assert not any(h.endswith("hn_spectral_lds.inc") for h in build.HEADERS)
    assert all(os.path.exists(h) for h in build.HEADERS) and all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.SOURCES)


def _ratios(n, tables=None):
    """error / bar of the restated fp32 algorithm: the four probes, then the two extra mode fields."""
    c, x = SP.forward_case(n), MP.extra_case(n)
    t = tables or MP.restated_tables(n)
    got = SP.apply_each(lambda u: MP.restated_laplacian(u, n, tables=t), n, c["u"])
    extra = SP.apply_each(lambda u: MP.restated_laplacian(u, n, tables=t), n, x["u"])
    assert got.dtype == torch.float32 and c["lap"].dtype == torch.float64
    return torch.cat([SP.errors(got, c["lap"]) / c["bar_lap"], SP.errors(extra, x["lap"]) / x["bar_lap"]])


@pytest.mark.parametrize("n", [144, 400, 1040, 2032])
def test_fp32_restatement_meets_the_bar_with_a_factor_three_to_spare(n):
    assert MP.spectral_route(n, mixed=1)[0] == "mixed"
    r = _ratios(n)
    print(f"MIXED n={n} = {MP.factor(n)[0]} * {MP.factor(n)[1]}: restated fp32 algorithm, error / bar: "
          + ", ".join(f"{nm} {float(v):.3f}" for nm, v in zip(SP.PROBES + MP.EXTRA_NAMES, r)))
    assert bool((3 * r <= 1.0).all()), r.tolist()


def test_one_swapped_entry_of_the_permuted_k_table_is_caught_by_the_extra_modes():
    n = 400
    p, q = MP.factor(n)
    j = 2 * q + p                                    # a frequency only the extra mode fields carry
    assert j in MP.extra_mode_indices(n) and j not in SP.mode_indices(n)
    r = _ratios(n, MP.mutate_k1p_entry(MP.restated_tables(n), j))
    print(f"MIXED n={n}, permuted k entry of frequency {j} swapped with its neighbour: error / bar "
          + ", ".join(f"{nm} {float(v):.2f}" for nm, v in zip(SP.PROBES + MP.EXTRA_NAMES, r)))
    assert float(r[4]) > 10.0 and float(r[5]) > 10.0


def test_extra_mode_fields_are_single_modes_per_line():
    for n in (144, 1152):
        u = MP.extra_mode_field(n)
        js = MP.extra_mode_indices(n)
        p, q = MP.factor(n)
        assert {p, q, q - 1, q + 1, 2 * q + p, n - q, n - p, p * q // 2, q * ((p - 1) // 2)} == set(js)
        spec = torch.fft.fft(torch.complex(u[0], u[1]).to(torch.complex128), dim=-1).abs() / n
        for i in range(n):
            assert abs(float(spec[i, js[i % len(js)]]) - 1.0) < 1e-6
        assert torch.equal(MP.extra_mode_field(n, along_y=True), u.transpose(-1, -2))


def test_launch_shapes_named_by_the_gpu_test():
    """The (n, batch) pairs test_spectral_mixed_gpu.py uses for "a sample's bits do not depend on its batch" hit different lines per block."""
    assert [MP.mixed_lines(144, 4, b) for b in (1, 3, 33, 64)] == [1, 1, 8, 16] and [MP.mixed_lines(144, 3, b) for b in (1, 3, 33, 64)] == [1, 1, 8, 16]
    assert MP.mixed_lines(1040, 4, 1) == 2
    assert [MP.mixed_lines(576, 4, b) for b in (1, 5)] == [1, 4]
    assert MP.mixed_lines(144, 4, 1000) == 16 and MP.mixed_lines(2032, 4, 1000) == 1
    # the dynamic LDS of every mixed size stays within the attribute build_axis sets
    for n in MP.legal_sizes() + SP.pfa_sizes():
        name, p, q = MP.spectral_route(n, pfa=0, mixed=1)
        if name == "mixed":
            assert (MP.mixed_lines(n, 4, 10 ** 6) * 4 * n + p + q) * 8 <= 96 * 1024, n
