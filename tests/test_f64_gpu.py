"""Float64 residual check on the GPU: hn_laplacian_f64 / hn_residual_f64 and IterativeSolver.verify().  Needs a real MI355X.

Expected values: the float64 reference formulation -- the oracle's spectral functions on float64 tensors with float64 tables (what the reference computes
after ``solver.double()``), evaluated here on the CPU from seeded inputs, once per size -- and, at n = 16 and 48, the oracle's independent float64 assembly
of the same operator as an explicit matrix.

Bar: max abs error <= 1e-11 * max|expected|.  Derived, not measured: an output is a sum of n <= 2048 products, rounding ~ n * 2^-53 ~ 2e-13 relative to
the largest term; 1e-11 leaves a factor of about 50."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PML, SIGMA_MAX, K = 8, 2.0, 1.0
BAR = 1e-11
# n = 16: the smallest legal size, one tile or less; 48: no power of two, tile remainders in both directions; 96: the training size; 144: the size whose
# fp32 path is the dense fallback; 256 with batch 2: several tiles and the batch stride.  src_batch 1 and B at n = 48.
CASES = [(16, 1, 1), (48, 2, 1), (48, 2, 2), (96, 1, 1), (144, 1, 1), (256, 2, 1)]
_cache = {}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def case(n, b, sb):
    """Seeded inputs (fp32-representable, so the fp32 path can be given the same problem) and the CPU float64 reference, computed once."""
    key = (n, b, sb)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 + 7 * n + 3 * b + sb)
        wf = torch.randn(b, 2, n, n, generator=g, dtype=torch.float32).double()
        sos = (1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float32))
        k_sq = ((1.0 / sos) ** 2).double()
        src = torch.randn(sb, 2, n, n, generator=g, dtype=torch.float32).double()
        t64 = O.SpectralTables(n, PML, SIGMA_MAX, K, dtype=torch.float64)
        lap = O.apply_laplacian(wf, t64).contiguous()
        res = O.get_residual(wf, k_sq, src, t64).contiguous()
        assert lap.dtype == res.dtype == torch.float64
        _cache[key] = dict(wf=wf, k_sq=k_sq, src=src, lap=lap, res=res)
    return _cache[key]


@pytest.fixture(scope="module")
def eng():
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    yield e
    e.close()


@pytest.fixture(scope="module")
def solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    return s


def _rel(got, want):
    err, scale = float((got.cpu() - want).abs().max()), float(want.abs().max())
    return err / scale


@pytest.mark.parametrize("n,b,sb", CASES)
def test_laplacian_and_residual_match_the_float64_reference(eng, n, b, sb):
    c = case(n, b, sb)
    eng.set_domain(n, PML, SIGMA_MAX, K)
    wf, k_sq, src = (c[k].to(DEV) for k in ("wf", "k_sq", "src"))
    lap = eng.laplacian64(wf)
    res, _ = eng.residual64(wf, k_sq, src)
    assert lap.dtype == res.dtype == torch.float64
    e_lap, e_res = _rel(lap, c["lap"]), _rel(res, c["res"])
    print(f"n={n} b={b} src_batch={sb}: laplacian {e_lap:.3e}, residual {e_res:.3e} of max|expected|")
    assert e_lap <= BAR and e_res <= BAR, (e_lap, e_res)


@pytest.mark.parametrize("n,b,sb", [(16, 1, 1), (48, 2, 1)])
def test_residual_matches_the_assembled_helmholtz_matrix(eng, n, b, sb):
    """M u - src with the oracle's explicit complex128 system matrix (an independent float64 assembly of the same operator)."""
    c = case(n, b, sb)
    eng.set_domain(n, PML, SIGMA_MAX, K)
    res, _ = eng.residual64(*(c[k].to(DEV) for k in ("wf", "k_sq", "src")))
    lap = eng.laplacian64(c["wf"].to(DEV))
    for i in range(b):
        k_sq = c["k_sq"][i, 0].numpy()
        u = (c["wf"][i, 0].numpy() + 1j * c["wf"][i, 1].numpy()).reshape(-1)
        s = c["src"][0 if sb == 1 else i]
        mat = O.assemble_helmholtz_matrix(k_sq, PML, SIGMA_MAX, K)
        want = (mat @ u - (s[0].numpy() + 1j * s[1].numpy()).reshape(-1)).reshape(n, n)
        got = res[i].cpu().numpy()
        err = max(np.abs(got[0] - want.real).max(), np.abs(got[1] - want.imag).max())
        assert err <= BAR * np.abs(want).max(), (i, err, np.abs(want).max())
        want_l = ((mat - np.diag(k_sq.reshape(-1))) @ u).reshape(n, n)
        got_l = lap[i].cpu().numpy()
        err_l = max(np.abs(got_l[0] - want_l.real).max(), np.abs(got_l[1] - want_l.imag).max())
        assert err_l <= BAR * np.abs(want_l).max(), (i, err_l)


def test_it_is_float64_and_not_a_cast(eng):
    """At n = 96 the float64 result differs from the fp32 hn_residual of the same (fp32-representable) inputs by more than 1e-9 * max, and is closer to
    the float64 reference than the fp32 result is by at least a factor 1e3."""
    c = case(96, 1, 1)
    eng.set_domain(96, PML, SIGMA_MAX, K)
    wf, k_sq, src = (c[k].to(DEV) for k in ("wf", "k_sq", "src"))
    res64, _ = eng.residual64(wf, k_sq, src)
    res32 = eng.residual(wf.float(), k_sq.float(), src.float())
    assert torch.equal(wf.float().double(), wf) and torch.equal(k_sq.float().double(), k_sq)
    scale = float(c["res"].abs().max())
    apart = float((res64 - res32.double()).abs().max())
    err64 = float((res64.cpu() - c["res"]).abs().max())
    err32 = float((res32.double().cpu() - c["res"]).abs().max())
    print(f"n=96: |f64 - f32| {apart / scale:.3e}, f64 vs reference {err64 / scale:.3e}, f32 vs reference {err32 / scale:.3e} (of max|expected|)")
    assert apart > 1e-9 * scale
    assert err64 * 1e3 <= err32


@pytest.mark.parametrize("n,b,sb", [(48, 2, 2), (256, 2, 1)])
def test_rmse_is_the_rmse_of_the_returned_residual_and_reproducible(eng, n, b, sb):
    c = case(n, b, sb)
    eng.set_domain(n, PML, SIGMA_MAX, K)
    wf, k_sq, src = (c[k].to(DEV) for k in ("wf", "k_sq", "src"))
    res, rmse = eng.residual64(wf, k_sq, src)
    want = res.pow(2).mean((1, 2, 3)).sqrt()
    assert rmse.dtype == torch.float64 and rmse.shape == (b,)
    assert float(((rmse - want).abs() / want).max()) <= 1e-14
    res2, rmse2 = eng.residual64(wf, k_sq, src)
    assert torch.equal(rmse, rmse2) and torch.equal(res, res2)
    only_rmse = eng.residual64(wf, k_sq, src, want_res=False)
    only_res = eng.residual64(wf, k_sq, src, want_rmse=False)
    assert only_rmse[0] is None and torch.equal(only_rmse[1], rmse)
    assert only_res[1] is None and torch.equal(only_res[0], res)


def test_argument_and_state_errors(eng):
    from helmnet_amd.engine import Engine
    c = case(16, 1, 1)
    eng.set_domain(16, PML, SIGMA_MAX, K)
    lib = eng.lib
    wf, k_sq, src = (c[k].to(DEV) for k in ("wf", "k_sq", "src"))
    out, rmse = torch.empty_like(wf), torch.empty(1, device=DEV, dtype=torch.float64)
    stream = eng._stream()
    assert lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 1, None, None, 1, stream) == -1      # both NULL
    assert lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 1, _ptr(wf), _ptr(rmse), 1, stream) == -1   # wf aliases res
    assert lib.hn_laplacian_f64(eng.ctx, _ptr(wf), _ptr(wf), 1, stream) == -1
    both = torch.zeros(2 * wf.numel(), device=DEV, dtype=torch.float64)
    assert lib.hn_laplacian_f64(eng.ctx, _ptr(both[: wf.numel()]), _ptr(both[wf.numel() // 2:]), 1, stream) == -1   # out overlaps half of wf
    assert lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 2, _ptr(out), None, 1, stream) == -1   # src_batch neither 1 nor B
    assert lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 1, _ptr(out), _ptr(rmse), 1, stream) == 0
    with pytest.raises(ValueError):
        eng.residual64(wf, k_sq, src, want_res=False, want_rmse=False)
    with pytest.raises(TypeError):
        eng.residual64(wf.float(), k_sq, src)
    with pytest.raises(TypeError):
        eng.laplacian64(wf.float())
    with pytest.raises(ValueError):
        eng.laplacian64(wf[:, :, :, :8])
    fresh = Engine(DEV)                                          # no hn_set_domain yet
    try:
        assert lib.hn_residual_f64(fresh.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 1, _ptr(out), _ptr(rmse), 1, stream) == -2
        assert lib.hn_laplacian_f64(fresh.ctx, _ptr(wf), _ptr(out), 1, stream) == -2
    finally:
        fresh.close()
    torch.cuda.synchronize()


def test_tables_follow_the_domain(eng):
    """96 -> 48 -> 96 on one context: the same bits for 96 both times, and 48 in between is right (tables rebuilt and freed with the domain)."""
    c96, c48 = case(96, 1, 1), case(48, 2, 1)
    args96 = [c96[k].to(DEV) for k in ("wf", "k_sq", "src")]
    args48 = [c48[k].to(DEV) for k in ("wf", "k_sq", "src")]
    eng.set_domain(96, PML, SIGMA_MAX, K)
    res_a, rmse_a = eng.residual64(*args96)
    eng.set_domain(48, PML, SIGMA_MAX, K)
    res_48, _ = eng.residual64(*args48)
    eng.set_domain(96, PML, SIGMA_MAX, K)
    res_b, rmse_b = eng.residual64(*args96)
    assert torch.equal(res_a, res_b) and torch.equal(rmse_a, rmse_b)
    assert _rel(res_48, c48["res"]) <= BAR and _rel(res_b, c96["res"]) <= BAR


def test_fp32_step_is_unaffected_by_float64_calls(solver):
    """An fp32 solve between two float64 calls gives bit-identical wavefields to a context that never made a float64 call."""
    from helmnet_amd import IterativeSolver
    from helmnet_amd.phantoms import ring_sos_batch
    plain = IterativeSolver.from_exported_weights()
    plain.freeze()
    plain.to(DEV)
    sos = torch.from_numpy(ring_sos_batch(96, 2, seed=5)).to(DEV)
    for s in (solver, plain):
        s.set_domain_size(96, source_location=[82, 48])
    want = plain.forward(sos, num_iterations=5, residuals="norms")
    k_sq = solver.get_initials(sos)[0]
    first = solver.get_residual64(want["wavefields"][0], k_sq)
    got = solver.forward(sos, num_iterations=5, residuals="norms")
    second = solver.get_residual64(want["wavefields"][0], k_sq)
    assert torch.equal(got["wavefields"][0], want["wavefields"][0])
    # (the norms of hn_step are sums of float atomics: two runs of ONE context agree to 1e-5 relative, not bit for bit -- INTEGRATION section 7)
    assert float((got["residual_norms"] / want["residual_norms"] - 1).abs().max()) <= 1e-5
    assert torch.equal(first, second) and first.dtype == torch.float64


def test_calls_are_capturable_once_the_tables_exist(eng):
    c = case(48, 2, 2)
    wf, k_sq, src = (c[k].to(DEV) for k in ("wf", "k_sq", "src"))
    out, rmse = torch.empty_like(wf), torch.empty(2, device=DEV, dtype=torch.float64)
    eng.set_domain(16, PML, SIGMA_MAX, K)
    eng.set_domain(48, PML, SIGMA_MAX, K)                          # a fresh domain: no float64 tables yet
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rmse.zero_()
            rc = eng.lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 2, _ptr(out), _ptr(rmse), 2, eng._stream())
        assert rc == -2                                            # would have to build the tables: refused before anything is enqueued
        want_res, want_rmse = eng.residual64(wf, k_sq, src)        # eager: builds them
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = eng.lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 2, _ptr(out), _ptr(rmse), 2, eng._stream())
        assert rc == 0
        out.zero_()
        rmse.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, want_res) and torch.equal(rmse, want_rmse)


def test_verify_reports_both_norms_and_the_evaluator_floor(solver):
    from helmnet_amd.phantoms import ring_sos_batch
    n, hp = 96, solver.hparams
    solver.set_domain_size(n, source_location=[82, 48])
    sos = torch.from_numpy(ring_sos_batch(n, 2, seed=11)).to(DEV)
    out = solver.forward(sos, num_iterations=20, residuals="norms")
    wf = out["wavefields"][0]
    v = solver.verify(wf, sos_maps=sos)
    assert set(v) == {"residual_norm64", "residual_norm32", "evaluator_error"}
    assert v["residual_norm64"].dtype == torch.float64 and v["residual_norm64"].shape == (2,)
    last = out["residual_norms"][-1]
    assert float(((v["residual_norm32"] - last).abs() / last).max()) <= 1e-5
    # the CPU float64 reference residual of the same wavefield, for the fp32 k_sq and source the solver ran
    k_sq = solver.get_initials(sos)[0]
    t64 = O.SpectralTables(n, int(hp.PMLsize), float(hp.sigma_max), float(hp.k), dtype=torch.float64)
    ref = O.get_residual(wf.double().cpu(), k_sq.double().cpu(), solver.source.detach().double().cpu(), t64)
    ref_norm = ref.pow(2).mean((1, 2, 3)).sqrt()
    rel = float(((v["residual_norm64"].cpu() - ref_norm).abs() / ref_norm).max())
    print(f"verify: norm64 {v['residual_norm64'].tolist()}, norm32 {v['residual_norm32'].tolist()}, evaluator error {v['evaluator_error'].tolist()}, "
          f"norm64 vs the CPU float64 reference {rel:.3e}")
    assert rel <= 1e-10
    assert bool((v["evaluator_error"] > 0).all()) and bool((v["evaluator_error"] < v["residual_norm64"]).all())
    r64 = solver.get_residual64(wf, k_sq)
    assert r64.dtype == torch.float64 and _rel(r64, ref) <= BAR
    v2 = solver.verify(wf, k_sq=k_sq)
    assert torch.equal(v["residual_norm64"], v2["residual_norm64"]) and torch.equal(v["evaluator_error"], v2["evaluator_error"])
    assert float((v2["residual_norm32"] / v["residual_norm32"] - 1).abs().max()) <= 1e-5      # hn_rmse adds with float atomics
    with pytest.raises(ValueError):
        solver.verify(wf)
    with pytest.raises(ValueError):
        solver.verify(wf, sos_maps=sos, k_sq=k_sq)
    with pytest.raises(RuntimeError):
        solver.verify(wf.clone().requires_grad_(True), k_sq=k_sq)


def test_solve_to_tolerance_verify_is_opt_in(solver):
    from helmnet_amd.phantoms import ring_sos_batch
    solver.set_domain_size(96, source_location=[82, 48])
    sos = torch.from_numpy(ring_sos_batch(96, 2, seed=11)).to(DEV)
    base = solver.solve_to_tolerance(sos, tol=1e-30, max_iterations=10, check_every=5)
    assert set(base) == {"wavefield", "residual", "residual_norms", "iterations", "converged"}
    more = solver.solve_to_tolerance(sos, tol=1e-30, max_iterations=10, check_every=5, verify=True)
    assert set(more) == set(base) | {"residual_norm64", "residual_norm32", "evaluator_error", "converged64"}
    assert torch.equal(more["wavefield"], base["wavefield"]) and torch.equal(more["residual"], base["residual"])
    assert float((more["residual_norms"] / base["residual_norms"] - 1).abs().max()) <= 1e-5   # hn_step's norms are sums of float atomics
    assert more["converged64"] is False and more["converged"] is False
    loose = solver.solve_to_tolerance(sos, tol=1e30, max_iterations=10, check_every=5, verify=True)
    assert loose["converged"] is True and loose["converged64"] is True
