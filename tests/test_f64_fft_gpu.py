"""The FFT route of the float64 operator on the GPU (HN_OPT_F64_FFT 1, hn_f64_fft.hip): hn_laplacian_f64 / hn_residual_f64 and everything behind
f64_apply.  Needs a real MI355X.

Expected values as in test_f64_gpu.py: the oracle's spectral functions on float64 tensors with float64 tables, evaluated on the CPU from seeded
fp32-representable inputs, once per case; at n = 16 and 48 also the oracle's explicit-matrix assembly.

Bars.  Reference: max abs error <= 1e-11 * max|expected| (test_f64_gpu.py's derived bar; a transform's rounding, O(log n) * 2^-53, is below the dense
sum's).  Route against route: 2e-11 (triangle inequality).  RMSE against the returned field: 1e-14 relative.  The solver loop: 1e-10 * max
(test_f64_solver_gpu.py's bar)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import helmnet_oracle as O
from test_f64_gpu import case, _ptr, _rel, DEV, PML, SIGMA_MAX, K, BAR

pytestmark = pytest.mark.gpu

# 16: smallest, P = 1; 64; 48 x 2 with a per-sample source: P = 3; 80 .. 208: P = 5, 7, 9, 11 (first prime above 8), 13; 272: P = 17, Q = 16; 256 x 2;
# 1536: Q = 512 with four buffers; 2032: P = 127, the longest four-buffer line; 2048: the longest line
CASES = [(16, 1, 1), (64, 1, 1), (48, 2, 2), (80, 1, 1), (112, 1, 1), (144, 1, 1), (176, 1, 1), (208, 1, 1), (272, 1, 1), (256, 2, 1), (1536, 1, 1),
         (2032, 1, 1), (2048, 1, 1)]
DEPTH = 4


@pytest.fixture(scope="module")
def eng():
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    yield e
    e.close()


def _domain(eng, n, fft=1):
    eng.set_domain(n, PML, SIGMA_MAX, K)
    eng.set_option("f64_fft", fft)


def _dev(c):
    return tuple(c[k].to(DEV) for k in ("wf", "k_sq", "src"))


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n,b,sb", CASES)
def test_fft_route_matches_the_float64_reference(eng, n, b, sb):
    from helmnet_amd.laplacian import f64_route
    c = case(n, b, sb)
    _domain(eng, n)
    wf, k_sq, src = _dev(c)
    lap = eng.laplacian64(wf)
    res, _ = eng.residual64(wf, k_sq, src)
    assert eng.counter("f64_route") == 2 and lap.dtype == res.dtype == torch.float64
    e_lap, e_res = _rel(lap, c["lap"]), _rel(res, c["res"])
    print(f"n={n} {f64_route(n, 1)} b={b} src_batch={sb}: laplacian {e_lap:.3e}, residual {e_res:.3e} of max|expected|")
    assert e_lap <= BAR and e_res <= BAR, (e_lap, e_res)


@pytest.mark.parametrize("n,b,sb", [(16, 1, 1), (48, 2, 2)])
def test_fft_route_matches_the_assembled_helmholtz_matrix(eng, n, b, sb):
    c = case(n, b, sb)
    _domain(eng, n)
    wf, k_sq, src = _dev(c)
    res, _ = eng.residual64(wf, k_sq, src)
    lap = eng.laplacian64(wf)
    for i in range(b):
        kq = c["k_sq"][i, 0].numpy()
        u = (c["wf"][i, 0].numpy() + 1j * c["wf"][i, 1].numpy()).reshape(-1)
        s = c["src"][0 if sb == 1 else i]
        mat = O.assemble_helmholtz_matrix(kq, PML, SIGMA_MAX, K)
        want = (mat @ u - (s[0].numpy() + 1j * s[1].numpy()).reshape(-1)).reshape(n, n)
        got = res[i].cpu().numpy()
        err = max(np.abs(got[0] - want.real).max(), np.abs(got[1] - want.imag).max())
        assert err <= BAR * np.abs(want).max(), (i, err, np.abs(want).max())
        want_l = ((mat - np.diag(kq.reshape(-1))) @ u).reshape(n, n)
        got_l = lap[i].cpu().numpy()
        err_l = max(np.abs(got_l[0] - want_l.real).max(), np.abs(got_l[1] - want_l.imag).max())
        assert err_l <= BAR * np.abs(want_l).max(), (i, err_l)


# ---------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n,b,sb", [(48, 2, 2), (144, 1, 1), (256, 2, 1), (2048, 1, 1)])
def test_the_two_routes_agree_and_their_tables_coexist(eng, n, b, sb):
    c = case(n, b, sb)
    wf, k_sq, src = _dev(c)
    _domain(eng, n, fft=0)
    dense_res, dense_rmse = eng.residual64(wf, k_sq, src)
    dense_lap = eng.laplacian64(wf)
    eng.set_option("f64_fft", 1)
    fft_res, fft_rmse = eng.residual64(wf, k_sq, src)
    fft_lap = eng.laplacian64(wf)
    eng.set_option("f64_fft", 0)
    again_res, again_rmse = eng.residual64(wf, k_sq, src)
    assert torch.equal(again_res, dense_res) and torch.equal(again_rmse, dense_rmse) and torch.equal(eng.laplacian64(wf), dense_lap)
    scale_r, scale_l = float(dense_res.abs().max()), float(dense_lap.abs().max())
    d_res, d_lap = float((fft_res - dense_res).abs().max()) / scale_r, float((fft_lap - dense_lap).abs().max()) / scale_l
    d_rmse = float(((fft_rmse - dense_rmse).abs() / dense_rmse).max())
    print(f"n={n}: FFT route vs dense route: residual {d_res:.3e}, laplacian {d_lap:.3e} of max, rmse {d_rmse:.3e} relative")
    assert d_res <= 2 * BAR and d_lap <= 2 * BAR and d_rmse <= 2 * BAR


# ---------------------------------------------------------------------------------------------- 3
def test_counter_tells_the_route_of_the_last_call(eng):
    c = case(16, 1, 1)
    wf = c["wf"].to(DEV)
    _domain(eng, 16, fft=0)
    assert eng.counter("f64_route") == 0
    eng.laplacian64(wf)
    assert eng.counter("f64_route") == 1
    eng.set_option("f64_fft", 1)
    assert eng.counter("f64_route") == 1            # the option alone changes nothing: the counter is the last CALL's route
    eng.laplacian64(wf)
    assert eng.counter("f64_route") == 2
    eng.set_domain(16, PML, SIGMA_MAX, K)
    assert eng.counter("f64_route") == 0
    eng.laplacian64(wf)                             # the option outlives the domain
    assert eng.counter("f64_route") == 2


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n,b,sb", [(48, 2, 2), (256, 2, 1)])
def test_rmse_is_the_rmse_of_the_returned_residual_and_reproducible(eng, n, b, sb):
    c = case(n, b, sb)
    _domain(eng, n)
    wf, k_sq, src = _dev(c)
    res, rmse = eng.residual64(wf, k_sq, src)
    want = res.pow(2).mean((1, 2, 3)).sqrt()
    assert rmse.dtype == torch.float64 and rmse.shape == (b,)
    assert float(((rmse - want).abs() / want).max()) <= 1e-14
    res2, rmse2 = eng.residual64(wf, k_sq, src)
    assert torch.equal(rmse, rmse2) and torch.equal(res, res2)
    only_rmse = eng.residual64(wf, k_sq, src, want_res=False)            # res == NULL: the column pass writes the library's intermediate field
    only_res = eng.residual64(wf, k_sq, src, want_rmse=False)
    assert only_rmse[0] is None and torch.equal(only_rmse[1], rmse)
    assert only_res[1] is None and torch.equal(only_res[0], res)


# (256, 8): the launch is large enough for four lines per block, where the sample alone runs one -- the rule of lines_per_block (hn_f64_fft.hip)
@pytest.mark.parametrize("n,batch", [(48, 3), (256, 3), (256, 8)])
def test_a_samples_bits_do_not_depend_on_its_batch(eng, n, batch):
    g = torch.Generator().manual_seed(4000 + n + batch)
    wf = torch.randn(batch, 2, n, n, generator=g, dtype=torch.float32).double().to(DEV)
    k_sq = (1.0 / (1.0 + torch.rand(batch, 1, n, n, generator=g, dtype=torch.float32)) ** 2).double().to(DEV)
    src = torch.randn(batch, 2, n, n, generator=g, dtype=torch.float32).double().to(DEV)
    _domain(eng, n)
    res, rmse = eng.residual64(wf, k_sq, src)
    rmse_only = eng.residual64(wf, k_sq, src, want_res=False)[1]
    for i in (0, batch - 1):
        res1, rmse1 = eng.residual64(wf[i:i + 1].contiguous(), k_sq[i:i + 1].contiguous(), src[i:i + 1].contiguous())
        assert torch.equal(res1[0], res[i]) and torch.equal(rmse1[0], rmse[i]) and torch.equal(rmse_only[i], rmse[i])


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("sb", [1, 2])
def test_broadcast_and_per_sample_source(eng, sb):
    c = case(48, 2, sb)
    _domain(eng, 48)
    res, rmse = eng.residual64(*_dev(c))
    assert _rel(res, c["res"]) <= BAR
    want = c["res"].pow(2).mean((1, 2, 3)).sqrt()
    assert float(((rmse.cpu() - want).abs() / want).max()) <= BAR


# ---------------------------------------------------------------------------------------------- 6
def _off_by_one_double(t):
    """The same values in a tensor that starts one double into a larger allocation (8-byte aligned, no more)."""
    big = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    view = big[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 8
    return view


def test_caller_views_and_the_overlap_refusal(eng):
    n, b = 48, 2
    c = case(n, b, 2)
    _domain(eng, n)
    wf, k_sq, src = _dev(c)
    want_res, want_rmse = eng.residual64(wf, k_sq, src)
    want_lap = eng.laplacian64(wf)
    lib, stream = eng.lib, eng._stream()
    wf_v, k_sq_v, src_v = (_off_by_one_double(t) for t in (wf, k_sq, src))
    out_v, rmse_v = _off_by_one_double(torch.zeros_like(wf)), _off_by_one_double(torch.zeros(b, device=DEV, dtype=torch.float64))
    assert lib.hn_residual_f64(eng.ctx, _ptr(wf_v), _ptr(k_sq_v), _ptr(src_v), 2, _ptr(out_v), _ptr(rmse_v), b, stream) == 0
    assert torch.equal(out_v, want_res) and torch.equal(rmse_v, want_rmse)
    out_v.zero_()
    assert lib.hn_laplacian_f64(eng.ctx, _ptr(wf_v), _ptr(out_v), b, stream) == 0
    assert torch.equal(out_v, want_lap)
    # wf overlapping out: refused with nothing written
    both = torch.zeros(2 * wf.numel(), device=DEV, dtype=torch.float64)
    both[: wf.numel()].copy_(wf.reshape(-1))
    before = both.clone()
    assert lib.hn_laplacian_f64(eng.ctx, _ptr(both[: wf.numel()]), _ptr(both[wf.numel() // 2:]), b, stream) == -1
    assert lib.hn_residual_f64(eng.ctx, _ptr(both), _ptr(k_sq), _ptr(src), 2, _ptr(both), None, b, stream) == -1
    torch.cuda.synchronize()
    assert torch.equal(both, before)


# ---------------------------------------------------------------------------------------------- 7
def test_first_call_refuses_capture_and_later_calls_are_capturable(eng):
    c = case(48, 2, 2)
    wf, k_sq, src = _dev(c)
    out, rmse = torch.full_like(wf, 7.0), torch.empty(2, device=DEV, dtype=torch.float64)
    eng.set_domain(16, PML, SIGMA_MAX, K)
    _domain(eng, 48)                                               # a fresh domain: no FFT tables yet
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rmse.zero_()
            rc = eng.lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 2, _ptr(out), _ptr(rmse), 2, eng._stream())
        assert rc == -2                                            # would have to build the tables: refused before anything is enqueued
        graph.replay()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                            # the refused call left out untouched
        assert eng.counter("f64_route") == 0
        want_res, want_rmse = eng.residual64(wf, k_sq, src)        # eager: builds them
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc_none = eng.lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 2, None, _ptr(rmse), 2, eng._stream())
        assert rc_none == -2                                       # rmse only: the intermediate field does not exist yet
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = eng.lib.hn_residual_f64(eng.ctx, _ptr(wf), _ptr(k_sq), _ptr(src), 2, _ptr(out), _ptr(rmse), 2, eng._stream())
        assert rc == 0
        out.zero_()
        rmse.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, want_res) and torch.equal(rmse, want_rmse)


# ---------------------------------------------------------------------------------------------- 8
def test_step_f64_follows_the_oracle_on_the_fft_route(weights):
    from helmnet_amd.engine import Engine, pack_weights
    n, b, n_iter = 48, 2, 3
    g = torch.Generator().manual_seed(500 + n + 10 * b)
    sos = (1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float32)).double()
    src = O.point_source_map(n, [n // 2, n // 3], 10.0).float().double().contiguous()
    t64 = O.SpectralTables(n, PML, SIGMA_MAX, K, dtype=torch.float64)
    w64 = {k: v.double() for k, v in weights.items()}
    k_sq, wf = O.get_initials(sos, 1.0)
    states = [torch.zeros(b, 2, s, s, dtype=torch.float64) for s in O.state_dims(n, DEPTH)]
    res = O.get_residual(wf, k_sq, src, t64).contiguous()
    st0 = O.flatten_states(states)
    want = dict(wf=[], res=[], st=[], rmse=[])
    w, r = wf, res
    for _ in range(n_iter):
        w, r, states = O.single_step(w, k_sq, r, states, w64, src, t64, DEPTH)
        want["wf"].append(w)
        want["res"].append(r)
        want["st"].append(O.flatten_states(states))
        want["rmse"].append(O.test_loss_function(r))
    e = Engine(DEV)
    try:
        e.load_weights(pack_weights(weights, DEPTH, "prelu"), 8, DEPTH, 2, "prelu")
        _domain(e, n)
        new = lambda *shape: torch.full(shape, float("nan"), device=DEV, dtype=torch.float64)  # noqa: E731
        d_wf, d_res, d_st = wf.to(DEV).clone(), res.to(DEV).clone(), st0.to(DEV).clone()
        h = dict(res_hist=new(n_iter, b, 2, n, n), wf_hist=new(n_iter, b, 2, n, n), st_hist=new(n_iter, b, 2, d_st.shape[-1]), rmse_hist=new(n_iter, b))
        e.step64(d_wf, d_res, d_st, k_sq.to(DEV), src.to(DEV), n_iter, **h)
        assert e.counter("f64_route") == 2
        errs = {}
        for it in range(n_iter):
            errs[f"wf_hist[{it}]"] = _rel(h["wf_hist"][it], want["wf"][it])
            errs[f"res_hist[{it}]"] = _rel(h["res_hist"][it], want["res"][it])
            errs[f"st_hist[{it}]"] = _rel(h["st_hist"][it], want["st"][it])
            errs[f"rmse_hist[{it}]"] = float(((h["rmse_hist"][it].cpu() - want["rmse"][it]).abs() / want["rmse"][it]).max())
        worst = max(errs, key=errs.get)
        print(f"hn_step_f64 on the FFT route, n={n} b={b}: worst {worst} {errs[worst]:.3e} of max|expected|")
        assert errs[worst] <= 1e-10, (worst, errs[worst])
        assert torch.equal(d_wf, h["wf_hist"][-1]) and torch.equal(d_res, h["res_hist"][-1])
    finally:
        e.close()


def test_refine_cycle_reports_the_fft_routes_rmse(eng):
    n, b, restart = 48, 2, 4
    g = torch.Generator().manual_seed(48)
    k_sq = (1.0 / (1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float32)) ** 2).to(DEV)
    rhs = torch.randn(b, 2, n, n, generator=g, dtype=torch.float32).to(DEV)
    x0 = (0.01 * torch.randn(b, 2, n, n, generator=g, dtype=torch.float64)).to(DEV)
    _domain(eng, n)
    want = eng.residual64(x0, k_sq.double(), rhs.double(), want_res=False)[1]
    x = x0.clone()
    rmse64, _, k_used = eng.gmres_refine_cycle(x, k_sq, rhs, restart, 1e-12)
    assert eng.counter("f64_route") == 2
    assert torch.equal(rmse64, want)
    assert k_used.tolist() == [restart] * b and not torch.equal(x, x0)


def test_verify_agrees_between_the_routes():
    from helmnet_amd import IterativeSolver
    n = 256
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    s.set_domain_size(n, source_location=[200, 128])
    g = torch.Generator().manual_seed(256)
    wf = (0.1 * torch.randn(1, 2, n, n, generator=g, dtype=torch.float32)).to(DEV)
    k_sq = (1.0 / (1.0 + torch.rand(1, 1, n, n, generator=g, dtype=torch.float32)) ** 2).to(DEV)
    e = s.engine()
    e.set_option("f64_fft", 0)
    dense = s.verify(wf, k_sq=k_sq)["residual_norm64"]
    assert e.counter("f64_route") == 1
    e.set_option("f64_fft", 1)
    fft = s.verify(wf, k_sq=k_sq)["residual_norm64"]
    assert e.counter("f64_route") == 2
    e.set_option("f64_fft", 0)
    rel = float(((fft - dense).abs() / dense).max())
    print(f"verify at {n}: float64 norm, FFT route vs dense route {rel:.3e} relative")
    assert rel <= 1e-11


# ---------------------------------------------------------------------------------------------- 9
def test_a_bad_option_value_is_refused_and_changes_nothing(eng):
    wf = case(16, 1, 1)["wf"].to(DEV)
    for kept, route in ((1, 2), (0, 1)):
        _domain(eng, 16, fft=kept)
        for bad in (2, -1):
            with pytest.raises(ValueError, match="HN_OPT_F64_FFT must be 0 or 1"):      # HN_ERR_ARG
                eng.set_option("f64_fft", bad)
        eng.laplacian64(wf)
        assert eng.counter("f64_route") == route
