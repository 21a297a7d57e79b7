"""Rectangular H x W domains without a GPU: the tables helper of tests/rect_common.py is pinned against the oracle, and the Python surface
(point source, state bookkeeping, per-axis route, the solver's tables) is checked at (H, W).

    1  with H == W every tensor of ``RectTables`` equals ``O.SpectralTables``'s, bit for bit;
    2  in float64, ``O.apply_laplacian(u, RectTables(H, W))`` is M_H U + U M_W^T with M_n = ``O.axis_operator_matrix(n, ...)``, to 1e-12 of
       max |L u|: which axis is which, independently of the helper;
    3  the Python front end at (H, W), and ``set_domain_size(96)`` exactly as before.
"""
import numpy as np
import pytest
import torch

import rect_common as R
from oracle import helmnet_oracle as O

TABLES = ("kx", "ky", "kx_sq", "ky_sq", "ax", "bx", "ay", "by", "sigma_x", "sigma_y", "sigmas")


@pytest.mark.parametrize("n", [16, 96, 144])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_square_helper_tables_are_the_oracles(n, dtype):
    got, want = R.RectTables(n, n, *R.DOMAIN, dtype=dtype), O.SpectralTables(n, *R.DOMAIN, dtype=dtype)
    for name in TABLES:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.parametrize("h,w", [(16, 48), (80, 32), (144, 64)])
def test_rect_laplacian_is_one_axis_operator_per_axis(h, w):
    t = R.RectTables(h, w, *R.DOMAIN, dtype=torch.float64)
    assert tuple(t.kx.shape) == (1, h, w, 2) and tuple(t.sigmas.shape) == (2, h, w)
    rng = np.random.default_rng(100 * h + w)
    u = rng.standard_normal((h, w)) + 1j * rng.standard_normal((h, w))
    want = O.axis_operator_matrix(h, *R.DOMAIN) @ u + u @ O.axis_operator_matrix(w, *R.DOMAIN).T
    x = torch.from_numpy(np.stack([u.real, u.imag])[None])
    got = O.apply_laplacian(x, t)[0].numpy()
    err = np.abs((got[0] + 1j * got[1]) - want).max()
    print(f"{h}x{w}: |L u - (M_H U + U M_W^T)| / max|L u| = {err / np.abs(want).max():.2e}")
    assert err <= 1e-12 * np.abs(want).max()
    # sigma_x varies along the last axis with the profile of length w, sigma_y along the first with that of length h
    sw, _, _ = O.pml_profiles(w, *R.DOMAIN)
    sh, _, _ = O.pml_profiles(h, *R.DOMAIN)
    assert np.array_equal(t.sigmas[0].numpy(), np.broadcast_to(sw.astype(np.float32).astype(np.float64)[None, :], (h, w)))
    assert np.array_equal(t.sigmas[1].numpy(), np.broadcast_to(sh.astype(np.float32).astype(np.float64)[:, None], (h, w)))


def _solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    return s


def test_python_surface_at_h_by_w():
    from helmnet_amd.laplacian import spectral_route, spectral_route_rect
    h, w = 96, 160
    s = _solver()
    s.set_domain_size((h, w), source_location=[20, 90])
    assert s.hparams.domain_size == (h, w)
    # the point-source map: source.py generalised to (H, W)
    assert tuple(s.source.shape) == (1, 2, h, w)
    assert torch.equal(s.source.data, R.point_source_map(h, w, [20, 90], float(s.hparams.source_amplitude)))
    peak = int(s.source[0, 0].argmax())
    assert (peak // w, peak % w) == (20, 90)
    # state dimensions as pairs, flat-state length sum (H >> d)(W >> d)
    assert s.f.states_dimension == [(h >> d, w >> d) for d in range(4)]
    assert s.f.total_state_length == R.state_len(h, w) == sum((h >> d) * (w >> d) for d in range(4))
    assert s.f.state_boundaries[1] == [h * w, h * w + (h // 2) * (w // 2)]
    s.f.clear_states(torch.zeros(3, 2, h, w))
    assert [tuple(t.shape) for t in s.f.get_states()] == [(3, 2, h >> d, w >> d) for d in range(4)]
    flat = torch.arange(3 * 2 * s.f.total_state_length, dtype=torch.float32).reshape(3, 2, -1)
    s.f.set_states(flat, flatten=True)
    assert torch.equal(s.f.get_states(flatten=True), flat)
    assert torch.equal(s.f.get_states()[1], R.unflatten_states(flat, h, w)[1])
    # sigmas [2, H, W] and Lap's per-axis tables in the reference's [1, H, W, 2] layouts: the helper's, bit for bit
    t = R.RectTables(h, w, int(s.hparams.PMLsize), float(s.hparams.sigma_max), float(s.hparams.k))
    assert torch.equal(s.sigmas, t.sigmas)
    for name in TABLES[:8]:
        assert tuple(getattr(s.Lap, name).shape) == (1, h, w, 2) and torch.equal(getattr(s.Lap, name).data, getattr(t, name)), name
    # source maps [S, 2, H, W] and several locations
    s.set_multiple_sources([[20, 90], [40, 10]])
    assert tuple(s.source.shape) == (2, 2, h, w)
    s.set_domain_size((h, w), source_map=torch.ones(3, 2, h, w))
    assert tuple(s.source.shape) == (3, 2, h, w)
    assert tuple(s.test_loss_function(torch.ones(2, 2, h, w)).shape) == (2,)
    k_sq, wf = s.get_initials(torch.full((2, 1, h, w), 2.0))
    assert tuple(wf.shape) == (2, 2, h, w) and float(k_sq[0, 0, 0, 0]) == 0.25
    # the per-axis route function
    assert spectral_route_rect(h, w) == ("rectangular", (3, 32), (5, 32))
    assert spectral_route_rect(16, 2048) == ("rectangular", (1, 16), (1, 2048)) and spectral_route_rect(2032, 1040) == ("rectangular", (127, 16), (65, 16))
    for n in range(16, 2049, 16):
        p, q = spectral_route_rect(n, 16 if n != 16 else 32)[1]
        assert (p, q) == R.factor(n) and p * q == n and p % 2 == 1 and 1 <= p <= 127 and 16 <= q <= 2048 and q & (q - 1) == 0
    for bad in ((96, 96), (8, 64), (64, 2064), (40, 64)):
        with pytest.raises(ValueError):
            spectral_route_rect(*bad)
    assert spectral_route(96) == ("prime_factor", 3, 32)
    # what the rectangular path does not cover says so, without a GPU
    sos = torch.ones(1, 1, h, w)
    for call in (lambda: s.forward64(sos), lambda: s.gmres(sos), lambda: s.gmres64(sos), lambda: s.solve_many(sos, 1e-3), lambda: s.trainer(),
                 lambda: s.verify(torch.zeros(1, 2, h, w), sos_maps=sos), lambda: s.jvp(sos), lambda: s.set_unet_precision("fp16"),
                 lambda: s.reference_error(torch.zeros(1, 2, h, w), sos), lambda: s.deviation_from_float64(sos, 4, [2]),
                 lambda: s.solve_to_tolerance(sos, 1e-3, verify=True)):
        with pytest.raises(NotImplementedError, match="rectangular domain"):
            call()
    s.set_unet_precision("valu")
    # a pair with H == W is the int
    s.set_domain_size((96, 96), source_location=[20, 48])
    assert s.hparams.domain_size == 96 and s.f.states_dimension == [96, 48, 24, 12]


def test_set_domain_size_with_an_int_is_unchanged():
    a, b = _solver(), _solver()
    b.set_domain_size((64, 160), source_location=[10, 100])      # a rectangular domain in between leaves nothing behind
    for s in (a, b):
        s.set_domain_size(96, source_location=[20, 48])
    want_src = O.point_source_map(96, [20, 48], float(a.hparams.source_amplitude), float(a.hparams.omega), float(a.hparams.source_phase),
                                  bool(a.hparams.source_smoothing))
    t = O.SpectralTables(96, int(a.hparams.PMLsize), float(a.hparams.sigma_max), float(a.hparams.k))
    for s in (a, b):
        assert s.hparams.domain_size == 96 and isinstance(s.hparams.domain_size, int)
        assert s.f.states_dimension == [96, 48, 24, 12] and s.f.total_state_length == 96 ** 2 + 48 ** 2 + 24 ** 2 + 12 ** 2
        assert s.f.state_boundaries == [[0, 9216], [9216, 11520], [11520, 12096], [12096, 12240]]
        assert [enc.domain_size for enc in s.f.enc] == [96, 48, 24, 12]
        assert tuple(s.source.shape) == (1, 2, 96, 96) and torch.equal(s.source.data, want_src)
        assert torch.equal(s.sigmas, t.sigmas)
        for name in TABLES[:8]:
            assert torch.equal(getattr(s.Lap, name).data, getattr(t, name)), name
    assert dict(a.hparams) == dict(b.hparams)
