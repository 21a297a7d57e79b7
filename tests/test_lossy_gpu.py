"""Absorbing media (hn_residual_lossy, hn_step_lossy, hn_fgmres_cycle_lossy and the ``absorption`` keyword) against float64 references composed in
tests/lossy_common.py.  Needs a real MI355X.

Bars:
    operator        SP.BAR * (scale * max|u| + max(|k~^2| |u|) + max|src|): the rectangular test's bar with the complex magnitude; with k_sq_im = 0
                    twice that against hn_residual (two fp32 routes, each within one bar of the truth)
    one step        tests/test_rect_gpu.py's _vs_float64, imported: 1e-5 * max of each tensor, or 2 x the fp32 oracle's own distance above 5e-6
    free run        the first 20 RMSE rows within 2 % of the fp32 oracle's trace (test_rect_gpu.py's tier for R.oracle_loop); below 1e-4 after 200
                    iterations (the CPU oracle reached 2.3e-5: a factor of 4)
    GMRES           max|got - want| <= 2e-4 * max|want| against the complex float64 direct solve (test_hip_gmres_vs_float64_direct_solve's bar)
    exact           torch.equal; RMSE rows rtol 1e-5 (one atomicAdd per block)
"""
import ctypes

import numpy as np
import pytest
import torch

import lossy_common as LC
import rect_common as R
import spectral_probes as SP
from oracle import helmnet_oracle as O
from test_rect_gpu import _vs_float64

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3
NAN = float("nan")

# P = 1, 1, 3, 5, 7, 9, 13 (the smallest Q) as squares, and two rectangles
OPERATOR_SHAPES = [(16, 16), (32, 32), (48, 48), (80, 80), (112, 112), (144, 144), (208, 208), (32, 80), (96, 160)]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _err(e):
    return e.lib.hn_last_error(e.ctx).decode()


def _engine(h=None, w=None, blob=None):
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    if blob is not None:
        e.load_weights(blob, 8, 4, 2, "prelu")
    if h is not None:
        e.set_domain_rect(h, w, *R.DOMAIN)
    return e


@pytest.fixture(scope="module")
def blob(weights_np):
    from helmnet_amd.engine import pack_weights
    return pack_weights(weights_np, 4, "prelu")


@pytest.fixture(scope="module")
def eng(blob):
    e = _engine(blob=blob)
    yield e
    e.close()


def _solver(n, loc):
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    s.set_domain_size(n, source_location=loc)
    return s


def _planes(sos, alpha):
    """(k_sq, k_sq_im) in fp32 by the formulas, written out (the helper is pinned by tests/test_lossy_host.py)."""
    k = 1.0 / sos
    return (k ** 2 - alpha ** 2).contiguous(), (2.0 * k * alpha).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------ 1: operator
@pytest.mark.parametrize("h,w", OPERATOR_SHAPES)
def test_residual_lossy_matches_the_float64_oracle(eng, h, w):
    c = LC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    route = eng.counter("spectral_route")
    u, kq, ki = c["u"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV)
    assert bool((c["k_sq_im"][1] <= 0).all()) and bool((c["k_sq_im"][0] >= 0).all())      # one sample with the other sign
    got = {"lres1": eng.residual_lossy(u, kq, ki, c["src1"].to(DEV)), "lresb": eng.residual_lossy(u, kq, ki, c["srcb"].to(DEV))}
    worst = {}
    for name in got:
        assert not bool(torch.isnan(got[name]).any()), name
        ratio = SP.errors(got[name], c[name]) / c["bar_" + name]
        worst[name] = float(ratio.max())
        print(f"LOSSY {h}x{w} {name}: error / bar per probe " + ", ".join(f"{p} {float(r):.3f}" for p, r in zip(R.PROBES, ratio)))
    print(f"LOSSY {h}x{w} (P, Q) rows {R.factor(w)} columns {R.factor(h)}, lossless route {route}: worst error / bar {max(worst.values()):.3f}")
    assert max(worst.values()) <= 1.0, worst
    # k_sq_im = 0: the lossless residual to twice the (lossless) bar -- another factorisation on a square domain, so not bit for bit
    zero = torch.zeros_like(ki)
    for src, bar in ((c["src1"], c["bar_res1"]), (c["srcb"], c["bar_resb"])):
        a, b = eng.residual_lossy(u, kq, zero, src.to(DEV)), eng.residual(u, kq, src.to(DEV))
        ratio = SP.peak(a.cpu().double() - b.cpu().double()) / (2 * bar)
        print(f"LOSSY {h}x{w} k_sq_im = 0 against hn_residual (src batch {src.shape[0]}): error / (2 bar) " + ", ".join(f"{float(r):.3f}" for r in ratio))
        assert bool((ratio <= 1.0).all()), ratio.tolist()
    assert eng.counter("spectral_route") == route      # the domain is what it was: a square stays square


# ----------------------------------------------------------------------------------------------------------------- 2: one teacher-forced step
def _step_case(h, w, b):
    ti = R.teacher_inputs(h, w, b, 9100 + 7 * h + w)
    alpha = (0.1 * (ti["sos"] - 1.0)).contiguous()                 # 0 .. 0.1 nepers per grid point, pixel by pixel
    k_sq, k_im = _planes(ti["sos"], alpha)
    return ti, k_sq, k_im, R.point_source_map(h, w, [h // 4, w // 2], 10.0)


def _oracle_step(ti, k_sq, k_im, src, wts, h, w, dtype):
    t = R.tables(h, w, R.DOMAIN, dtype)
    wd = {k: v.to(dtype) for k, v in wts.items()}
    x = {k: v.to(dtype) for k, v in ti.items()}
    st = R.unflatten_states(x["states"], h, w)
    with torch.no_grad():
        wf, res, st2, d = LC.single_step(x["wf"], k_sq.to(dtype), k_im.to(dtype), x["res"], st, wd, src.to(dtype), t)
    return {"d": d, "wf": wf, "res": res, "states": O.flatten_states(st2)}


@pytest.mark.parametrize("h,w,b", [(96, 96, 2), (32, 80, 2)])
def test_one_teacher_forced_lossy_step_vs_float64(eng, weights, h, w, b):
    eng.set_domain_rect(h, w, *R.DOMAIN)
    ti, k_sq, k_im, src = _step_case(h, w, b)
    g = {k: v.to(DEV) for k, v in ti.items()}
    wf, res, st = g["wf"].clone(), g["res"].clone(), g["states"].clone()
    hist = [torch.full((1,) + tuple(t.shape), NAN, device=DEV) for t in (res, wf, st)]
    rmse = torch.full((1, b), NAN, device=DEV)
    eng.step_lossy(wf, res, st, k_sq.to(DEV), k_im.to(DEV), src.to(DEV), 1, hist[0], hist[1], hist[2], rmse)
    torch.cuda.synchronize()
    eng.check_async_errors()
    w64, w32 = (_oracle_step(ti, k_sq, k_im, src, weights, h, w, dt) for dt in (torch.float64, torch.float32))
    got = {"wf": wf, "res": res, "states": st}
    report, ok = [], []
    for k in ("wf", "res"):
        ok.append(_vs_float64(k, got[k], w64[k], w32[k], report))
    o = 0
    for d in range(4):
        lv = slice(o, o + (h >> d) * (w >> d))
        o = lv.stop
        ok.append(_vs_float64(f"state{d}", st[:, :, lv], w64["states"][:, :, lv], w32["states"][:, :, lv], report))
    print(f"LOSSY step {h}x{w}x{b}: " + "; ".join(report))
    assert all(ok), report
    # the lossless residual of the same wavefield is far from it: the imaginary plane is not ignored
    lossless = O.get_residual(w64["wf"], k_sq.double(), src.double(), R.tables(h, w))
    assert float((res.cpu().double() - w64["res"]).abs().max()) < 0.01 * float((lossless - w64["res"]).abs().max())
    want = eng.rmse(res)
    assert float(((rmse[0] - want).abs() / want).max()) <= 1e-5, (rmse.tolist(), want.tolist())
    assert torch.equal(hist[0][0], res) and torch.equal(hist[1][0], wf) and torch.equal(hist[2][0], st)


# ------------------------------------------------------------------------------------------------------------------------------ 3: free run
@pytest.mark.parametrize("a0", [0.02, 0.1])
def test_free_run_follows_the_oracle_and_converges(eng, weights, a0):
    from helmnet_amd.phantoms import ring_sos_batch
    n, b, loc = 96, 2, [20, 48]
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=3))
    alpha = LC.ring_alpha(sos, a0)
    _, tr32 = LC.oracle_loop(n, sos, alpha, 20, weights, torch.float32, loc)
    eng.set_domain(n, *R.DOMAIN)
    k_sq, k_im = (t.to(DEV) for t in _planes(sos, alpha))
    src = R.point_source_map(n, n, loc, 10.0).to(DEV)
    wf = torch.zeros(b, 2, n, n, device=DEV)
    res = eng.residual_lossy(wf, k_sq, k_im, src)
    st = torch.zeros(b, 2, eng.state_len, device=DEV)
    rmse = torch.full((200, b), NAN, device=DEV)
    eng.step_lossy(wf, res, st, k_sq, k_im, src, 200, rmse_hist=rmse)
    torch.cuda.synchronize()
    eng.check_async_errors()
    rel = ((rmse[:20].cpu().double() - tr32.double()).abs() / tr32.double()).max().item()
    rows = {k: [f"{v:.2e}" for v in rmse[k - 1].tolist()] for k in (10, 50, 100, 200)}
    print(f"LOSSY free run 96^2 a0={a0}: first 20 RMSE rows vs the fp32 oracle {rel:.2e}; RMSE at 10 / 50 / 100 / 200: {rows}")
    assert rel <= 0.02
    assert bool((rmse[-1] < 1e-4).all()), rmse[-1].tolist()
    true = eng.rmse(eng.residual_lossy(wf, k_sq, k_im, src))
    assert float(((true - rmse[-1]).abs() / true).max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------- 4: GMRES against the direct solve
@pytest.mark.parametrize("n,loc", [(32, [12, 16]), (48, [14, 24])])
def test_lossy_gmres_vs_float64_direct_solve(n, loc):
    from helmnet_amd.absorption import complex_k_sq
    from helmnet_amd.gmres import gmres
    s = _solver(n, loc)
    sos, alpha = LC.ring_medium(n, 0.1)
    out = gmres(s, sos.to(DEV), restart=40, max_outer=60, tol=2e-6, backend="hip", absorption=alpha.to(DEV))
    got = out["wavefield"].cpu().numpy()
    src = s.source.detach().cpu().numpy()[0]
    k_re, k_im = complex_k_sq(sos, alpha, 1.0)
    print("iterations per sample", out["iterations_per_sample"].tolist(), "converged", out["converged"], "cycles", out["cycles"])
    assert out["converged"]
    for b in range(2):
        want, _ = LC.direct_solve(k_re[b, 0].numpy(), k_im[b, 0].numpy(), src)
        err, scale = np.abs(got[b] - want).max(), np.abs(want).max()
        print(f"n={n} sample {b}: max|got - want| = {err:.3e}, bar {2e-4 * scale:.3e}")
        assert err <= 2e-4 * scale, (b, err, scale)
    s.engine().check_async_errors()


# ------------------------------------------------------------------------------------------------------------------ 5: learned preconditioner
def test_learned_preconditioner_on_a_lossy_medium():
    from helmnet_amd.absorption import complex_k_sq
    from helmnet_amd.phantoms import ring_sos_batch
    n = 96
    s = _solver(n, [20, 48])
    sos = torch.from_numpy(ring_sos_batch(n, 2, seed=3)).to(DEV)
    alpha = LC.ring_alpha(sos, 0.02)
    pre = s.gmres(sos, restart=40, max_cycles=200, tol=2e-6, absorption=alpha, precondition="learned")
    plain = s.gmres(sos, restart=40, max_cycles=200, tol=2e-6, absorption=alpha)
    print(f"LOSSY gmres 96^2 a0=0.02: learned {pre['cycles']} cycles ({pre['unet_evaluations']} UNet evaluations), plain {plain['cycles']} cycles")
    assert pre["converged"] and plain["converged"]
    assert pre["unet_evaluations"] == pre["cycles"] * 40 * 10 and plain["unet_evaluations"] == 0
    a, b = pre["wavefield"], plain["wavefield"]
    scale = float(b.abs().max())
    print(f"   max |learned - plain| = {float((a - b).abs().max()):.3e}, bar {4e-4 * scale:.3e}")
    assert float((a - b).abs().max()) <= 4e-4 * scale
    eng = s.engine()
    k_sq, k_im = complex_k_sq(sos, alpha, 1.0)
    for x in (a, b):
        assert float(eng.rmse(eng.residual_lossy(x, k_sq, k_im, s.source.detach().float().contiguous())).max()) < 2e-4
    eng.check_async_errors()


# ------------------------------------------------------------------------------------------------------------------------------ 6: refusals
def _raw_args(hw, b=2, restart=3):
    h, w = hw
    P = h * w
    new = lambda *shape: torch.full(shape, NAN, device=DEV)  # noqa: E731
    ti = R.teacher_inputs(h, w, b, 41)
    g = {k: v.to(DEV) for k, v in ti.items()}
    alpha = (0.1 * (g["sos"] - 1.0)).contiguous()
    k_sq, k_im = _planes(g["sos"], alpha)
    return dict(wf=g["wf"], res=g["res"].clone(), st=g["states"], k_sq=k_sq, k_im=k_im, src=R.point_source_map(h, w, [h // 4, w // 2], 10.0).to(DEV),
                out=new(b, 2, h, w), rmse_hist=new(1, b), basis=new(b, restart + 1, 2 * P), zbasis=new(b, restart, 2 * P), hess=new(b, restart + 1, restart, 2),
                rmse=new(restart + 1, b), k_used=torch.full((b,), -7, device=DEV, dtype=torch.int32))


def _residual(e, a, k_im, out=None):
    out = a["out"] if out is None else out
    return e.lib.hn_residual_lossy(e.ctx, _ptr(a["wf"]), _ptr(a["k_sq"]), _ptr(k_im), _ptr(a["src"]), 1, _ptr(out), a["wf"].shape[0], e._stream())


def _step(e, a, k_im, wf, res, st):
    return e.lib.hn_step_lossy(e.ctx, _ptr(wf), _ptr(res), _ptr(st), _ptr(a["k_sq"]), _ptr(k_im), _ptr(a["src"]), 1, wf.shape[0], 1, None, None, None,
                               _ptr(a["rmse_hist"]), e._stream())


def _cycle(e, a, k_im, x, iters=0):
    return e.lib.hn_fgmres_cycle_lossy(e.ctx, _ptr(x), _ptr(a["k_sq"]), _ptr(k_im), _ptr(a["src"]), 1, x.shape[0], 3, 0.0, iters, 1.0, _ptr(a["basis"]),
                                       _ptr(a["zbasis"]), _ptr(a["hess"]), _ptr(a["rmse"]), _ptr(a["k_used"]), e._stream())


OUTPUTS = ("out", "rmse_hist", "basis", "zbasis", "hess", "rmse", "k_used")


def _untouched(a):
    torch.cuda.synchronize()
    for k in OUTPUTS:
        t = a[k]
        assert bool((t == -7).all()) if t.dtype == torch.int32 else bool(torch.isnan(t).all()), k


def test_refusals_write_nothing(blob):
    n = 96
    e = _engine(n, n, blob)
    try:
        a = _raw_args((n, n))
        keep = {k: a[k].clone() for k in ("wf", "res", "st")}
        wf, res, st = a["wf"].clone(), a["res"].clone(), a["st"].clone()

        def inputs_unchanged():
            torch.cuda.synchronize()
            assert torch.equal(wf, keep["wf"]) and torch.equal(res, keep["res"]) and torch.equal(st, keep["st"])

        # k_sq_im = NULL: HN_ERR_ARG naming the lossless sibling
        for call, sibling in ((lambda: _residual(e, a, None), "hn_residual"), (lambda: _step(e, a, None, wf, res, st), "hn_step"),
                              (lambda: _cycle(e, a, None, wf), "hn_fgmres_cycle")):
            assert call() == ERR_ARG
            assert "k_sq_im is NULL" in _err(e) and _err(e).rstrip(")").endswith(" " + sibling), _err(e)
        _untouched(a)
        inputs_unchanged()
        # a k_sq_im that overlaps res (the last plane of res is the first of k_sq_im); for the cycle, one that lies in the basis
        P = n * n
        buf = torch.full((6 * P,), NAN, device=DEV)
        res_v, kim_v = buf[: 4 * P].view(2, 2, n, n), buf[3 * P: 5 * P].view(2, 1, n, n)
        assert _residual(e, a, kim_v, out=res_v) == ERR_ARG and "k_sq_im overlaps res" in _err(e), _err(e)
        assert _step(e, a, kim_v, wf, res_v, st) == ERR_ARG and "overlaps" in _err(e) and "k_sq_im" in _err(e), _err(e)
        assert _cycle(e, a, a["basis"].view(-1)[: 2 * P].view(2, 1, n, n), wf) == ERR_ARG and "k_sq_im overlaps basis" in _err(e), _err(e)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())
        _untouched(a)
        inputs_unchanged()
        # the first lossy call on a square domain under capture: HN_ERR_STATE, nothing enqueued
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = _residual(e, a, a["k_im"])
        torch.cuda.synchronize()
        assert rc == ERR_STATE and "capture" in _err(e), (rc, _err(e))
        _untouched(a)
        # ... and after an eager call the same call is captured and replayed
        eager = e.residual_lossy(a["wf"], a["k_sq"], a["k_im"], a["src"])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = _residual(e, a, a["k_im"])
            assert rc == OK, _err(e)
            graph.replay()
            torch.cuda.synchronize()
        assert torch.equal(a["out"], eager)
        a["out"].fill_(NAN)
        # HN_OPT_LANES 2
        e.set_option("lanes", 2)
        assert _step(e, a, a["k_im"], wf, res, st) == ERR_UNSUPPORTED and "HN_OPT_LANES" in _err(e), _err(e)
        e.set_option("lanes", 1)
        _untouched(a)
        inputs_unchanged()
        # the cycle on a rectangular domain
        e.set_domain_rect(32, 80, *R.DOMAIN)
        r = _raw_args((32, 80))
        x = r["wf"].clone()
        assert _cycle(e, r, r["k_im"], x) == ERR_UNSUPPORTED and "rectangular domain" in _err(e) and "32 x 80" in _err(e), _err(e)
        _untouched(r)
        assert torch.equal(x, r["wf"])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------- 7: no side effects on existing behaviour
def _lossless(e, n, b=2):
    ti = R.teacher_inputs(n, n, b, 300 + n)
    g = {k: v.to(DEV) for k, v in ti.items()}
    k_sq = ((1.0 / g["sos"]) ** 2).contiguous()
    src = R.point_source_map(n, n, [n // 4, n // 2], 10.0).to(DEV)
    res0 = e.residual(g["wf"], k_sq, src)
    wf, res, st = g["wf"].clone(), res0.clone(), g["states"].clone()
    hist = [torch.full((2,) + tuple(t.shape), NAN, device=DEV) for t in (res, wf, st)]
    rmse = torch.full((2, b), NAN, device=DEV)
    e.step(wf, res, st, k_sq, src, 2, hist[0], hist[1], hist[2], rmse)
    torch.cuda.synchronize()
    e.check_async_errors()
    return [res0, wf, res, st, rmse] + hist


def _same_lossless(got, want):
    for i, (p, q) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(p).any())
        if i == 4:      # the RMSE rows: one atomicAdd per block
            assert torch.allclose(p, q, rtol=1e-5, atol=0)
        else:
            assert torch.equal(p, q), i


@pytest.mark.parametrize("n,mixed", [pytest.param(96, 0, id="96"), pytest.param(144, 0, id="144"), pytest.param(144, 1, id="144-mixed")])
def test_lossy_calls_leave_the_lossless_entry_points_alone(blob, n, mixed):
    used, fresh = _engine(blob=blob), _engine(blob=blob)
    try:
        for e in (used, fresh):
            e.set_option("spectral_mixed", mixed)
            e.set_domain(n, *R.DOMAIN)
        route = fresh.counter("spectral_route")
        assert (route == 4) == bool(mixed)
        a = _raw_args((n, n))
        used.residual_lossy(a["wf"], a["k_sq"], a["k_im"], a["src"])
        wf, res, st = a["wf"].clone(), a["res"].clone(), a["st"].clone()
        used.step_lossy(wf, res, st, a["k_sq"], a["k_im"], a["src"], 2)
        x = a["wf"].clone()
        used.fgmres_cycle_lossy(x, a["k_sq"], a["k_im"], a["src"], 3, 0.0, 1, 1.0)
        torch.cuda.synchronize()
        used.check_async_errors()
        assert used.counter("spectral_route") == route
        _same_lossless(_lossless(used, n), _lossless(fresh, n))
    finally:
        used.close()
        fresh.close()


def test_one_line_axis_serves_the_mixed_route_and_the_lossy_operator(blob):
    """n = 144 = 9 * 16 with spectral_mixed 1: the lossless operator and the lossy one run on ONE set of line tables (ctx->sq_axis), built by
    hn_set_domain -- so the first lossy call may be captured -- and freed with the domain's tables, whatever the order of re-builds.  Every comparison
    is with an engine that has done nothing else."""
    n = 144
    used, mixed, dense = _engine(blob=blob), _engine(blob=blob), _engine(blob=blob)
    try:
        for e, opt in ((used, 1), (mixed, 1), (dense, 0)):
            e.set_option("spectral_mixed", opt)
            e.set_domain(n, *R.DOMAIN)
        assert used.counter("spectral_route") == mixed.counter("spectral_route") == 4 and dense.counter("spectral_route") == 3
        want_mixed, want_dense = _lossless(mixed, n), _lossless(dense, n)
        a = _raw_args((n, n))
        g = a["res"]
        want_vjp = mixed.residual_vjp(g, a["k_sq"])
        # the first lossy call of this engine, under capture: its tables are the mixed route's, nothing is left to build
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = _residual(used, a, a["k_im"])
            assert rc == OK, _err(used)
            _untouched(a)
            graph.replay()
            torch.cuda.synchronize()
        first = a["out"].clone()
        assert not bool(torch.isnan(first).any())
        assert torch.equal(used.residual_lossy(a["wf"], a["k_sq"], a["k_im"], a["src"]), first)
        _same_lossless(_lossless(used, n), want_mixed)
        # off the mixed route: the lossy operator re-builds the same tables at its first call, the lossless one is the dense operator
        used.set_option("spectral_mixed", 0)
        assert used.counter("spectral_route") == 3
        assert torch.equal(used.residual_lossy(a["wf"], a["k_sq"], a["k_im"], a["src"]), first)
        _same_lossless(_lossless(used, n), want_dense)
        # ... and back, with the axis the lossy call left replaced by the domain's own
        used.set_option("spectral_mixed", 1)
        assert used.counter("spectral_route") == 4
        _same_lossless(_lossless(used, n), want_mixed)
        assert torch.equal(used.residual_vjp(g, a["k_sq"]), want_vjp)
        # through a rectangular domain, which has axes of its own
        used.set_domain_rect(32, 80, *R.DOMAIN)
        assert used.counter("spectral_route") == 5
        used.set_domain(n, *R.DOMAIN)
        assert used.counter("spectral_route") == 4
        _same_lossless(_lossless(used, n), want_mixed)
        assert torch.equal(used.residual_lossy(a["wf"], a["k_sq"], a["k_im"], a["src"]), first)
        torch.cuda.synchronize()
        used.check_async_errors()
    finally:
        for e in (used, mixed, dense):
            e.close()


# ------------------------------------------------------------------------------------------------------------------------ 8: Python front end
def test_python_front_end():
    from helmnet_amd.phantoms import ring_sos_batch
    n = 96
    s = _solver(n, [20, 48])
    sos = torch.from_numpy(ring_sos_batch(n, 2, seed=3)).to(DEV)
    alpha = LC.ring_alpha(sos, 0.02)
    # absorption=None: the code path and the bits of before
    x, y = s.forward(sos, num_iterations=3), s.forward(sos, num_iterations=3, absorption=None)
    assert all(torch.equal(p, q) for k in ("wavefields", "residuals") for p, q in zip(x[k], y[k]))
    assert torch.allclose(x["residual_norms"], y["residual_norms"], rtol=1e-5, atol=0)      # the RMSE rows: one atomicAdd per block
    out = s.forward(sos, num_iterations=3, return_wavefields=True, return_states=True, absorption=alpha)
    assert set(out) == set(s.forward(sos, num_iterations=3, return_wavefields=True, return_states=True)) and out["last_iteration"] == 2
    assert all(tuple(t.shape) == (2, 2, n, n) for t in out["wavefields"] + out["residuals"]) and len(out["wavefields"]) == len(out["residuals"]) == 3
    assert tuple(out["states"][0].shape) == (2, 2, R.state_len(n, n)) and tuple(out["residual_norms"].shape) == (3, 2)
    assert not torch.equal(out["wavefields"][-1], x["wavefields"][-1])
    k_sq, k_im = _planes(sos, alpha)
    assert torch.equal(s.get_residual(out["wavefields"][-1], k_sq, k_sq_im=k_im), out["residuals"][-1])
    # a number is the uniform map
    u1 = s.forward(sos, num_iterations=2, absorption=0.02, residuals="last")
    u2 = s.forward(sos, num_iterations=2, absorption=torch.full_like(sos, 0.02), residuals="last")
    assert torch.equal(u1["wavefields"][0], u2["wavefields"][0])
    tol = s.solve_to_tolerance(sos, 1e-4, max_iterations=400, absorption=alpha)
    print(f"LOSSY python: solve_to_tolerance(1e-4) at 96^2, a0 = 0.02: {tol['iterations']} iterations, converged {tol['converged']}, "
          f"last rmse {tol['residual_norms'][-1].tolist()}")
    assert tol["converged"] and tol["iterations"] <= 400
    with pytest.raises(NotImplementedError, match="verify=True"):
        s.solve_to_tolerance(sos, 1e-4, max_iterations=400, verify=True, absorption=alpha)
    with pytest.raises(RuntimeError, match="grad"):
        s.forward(sos.clone().requires_grad_(True), num_iterations=2, absorption=alpha)
    s.engine().check_async_errors()
