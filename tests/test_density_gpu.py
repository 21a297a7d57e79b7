"""Heterogeneous density (hn_residual_medium, hn_step_medium, hn_fgmres_cycle_medium and the ``density`` keyword) against float64 references composed
in tests/density_common.py.  Needs a real MI355X.

Bars:
    operator        the lossy test's bar (the lossless one where k_sq_im is NULL) plus the new term's share under the same rule,
                    SP.BAR * max(|b_x q_x d_x u| + |b_y q_y d_y u|); the term itself is about 15 000 x the bar, so a dropped term, a wrong sign or
                    swapped planes cannot pass.  With q = 0: the constant-density sibling to twice its bar
    one step        tests/test_rect_gpu.py's _vs_float64, imported: 1e-5 * max of each tensor, or 2 x the fp32 oracle's own distance above 5e-6
    free run        the first 20 RMSE rows within 2 % of the fp32 oracle's trace; at most 1.3e-3 after 300 iterations (the CPU oracle reached 3.3e-4:
                    a factor of 4, the lossy test's margin)
    GMRES           max|got - want| <= 2e-4 * max|want| against the float64 direct solve of the assembled A_rho
    exact           torch.equal; RMSE rows rtol 1e-5 (one atomicAdd per block)
"""
import ctypes

import numpy as np
import pytest
import torch

import density_common as DC
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


# ------------------------------------------------------------------------------------------------------------------------------ 1: operator
@pytest.mark.parametrize("h,w", OPERATOR_SHAPES)
def test_residual_medium_matches_the_float64_oracle(eng, h, w):
    c = DC.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    route = eng.counter("spectral_route")
    u, kq, ki, q = (c[k].to(DEV) for k in ("u", "k_sq", "k_sq_im", "q"))
    assert float(c["q"].min()) < -0.39 and float(c["q"].max()) > 0.39
    src1, srcb = c["src1"].to(DEV), c["srcb"].to(DEV)
    got = {"mres1": eng.residual_medium(u, kq, ki, q, src1), "mresb": eng.residual_medium(u, kq, ki, q, srcb),
           "dres1": eng.residual_medium(u, kq, None, q, src1), "dresb": eng.residual_medium(u, kq, None, q, srcb)}
    worst = {}
    for name in got:
        assert not bool(torch.isnan(got[name]).any()), name
        ratio = SP.errors(got[name], c[name]) / c["bar_" + name]
        worst[name] = float(ratio.max())
        print(f"DENSITY {h}x{w} {name}: error / bar per probe " + ", ".join(f"{p} {float(r):.3f}" for p, r in zip(R.PROBES, ratio)))
    term_over_bar = float((SP.peak(c["term"]) / c["bar_mres1"]).min())
    print(f"DENSITY {h}x{w} (P, Q) rows {R.factor(w)} columns {R.factor(h)}, lossless route {route}: worst error / bar {max(worst.values()):.3f}; "
          f"the density term is at least {term_over_bar:.0f} x the bar")
    assert max(worst.values()) <= 1.0, worst
    assert term_over_bar > 100.0      # a dropped term, a wrong sign, swapped planes: hundreds of bars
    # q = 0: the constant-density siblings to twice their bar -- and whether bit for bit, which is reported, not asserted
    zero = torch.zeros_like(q)
    for src, bl, b0 in ((src1, c["bar_lres1"], c["bar_res1"]), (srcb, c["bar_lresb"], c["bar_resb"])):
        for k_im, sib, bar, name in ((ki, eng.residual_lossy(u, kq, ki, src), bl, "hn_residual_lossy"), (None, eng.residual(u, kq, src), b0, "hn_residual")):
            a = eng.residual_medium(u, kq, k_im, zero, src)
            ratio = SP.peak(a.cpu().double() - sib.cpu().double()) / (2 * bar)
            print(f"DENSITY {h}x{w} q = 0 against {name} (src batch {src.shape[0]}): error / (2 bar) " + ", ".join(f"{float(r):.3f}" for r in ratio)
                  + f"; bit-equal {torch.equal(a, sib)}")
            assert bool((ratio <= 1.0).all()), (name, ratio.tolist())
    assert eng.counter("spectral_route") == route      # the domain is what it was: a square stays square


# ----------------------------------------------------------------------------------------------------------------- 2: one teacher-forced step
def _step_case(h, w, b, lossy):
    ti = R.teacher_inputs(h, w, b, 9300 + 7 * h + w)
    k = 1.0 / ti["sos"]
    alpha = (0.1 * (ti["sos"] - 1.0)).contiguous()
    k_sq = (k ** 2 - alpha ** 2).contiguous() if lossy else (k ** 2).contiguous()
    k_im = (2.0 * k * alpha).contiguous() if lossy else None
    return ti, k_sq, k_im, DC.seeded_q(h, w, b), R.point_source_map(h, w, [h // 4, w // 2], 10.0)


def _oracle_step(ti, k_sq, k_im, q, src, wts, h, w, dtype):
    t = R.tables(h, w, R.DOMAIN, dtype)
    wd = {k: v.to(dtype) for k, v in wts.items()}
    x = {k: v.to(dtype) for k, v in ti.items()}
    st = R.unflatten_states(x["states"], h, w)
    with torch.no_grad():
        wf, res, st2, d = DC.single_step(x["wf"], k_sq.to(dtype), None if k_im is None else k_im.to(dtype), q.to(dtype), x["res"], st, wd, src.to(dtype), t)
    return {"d": d, "wf": wf, "res": res, "states": O.flatten_states(st2)}


@pytest.mark.parametrize("h,w,b,lossy", [(96, 96, 2, True), (96, 96, 2, False), (32, 80, 2, True), (32, 80, 2, False)])
def test_one_teacher_forced_medium_step_vs_float64(eng, weights, h, w, b, lossy):
    eng.set_domain_rect(h, w, *R.DOMAIN)
    ti, k_sq, k_im, q, src = _step_case(h, w, b, lossy)
    g = {k: v.to(DEV) for k, v in ti.items()}
    wf, res, st = g["wf"].clone(), g["res"].clone(), g["states"].clone()
    hist = [torch.full((1,) + tuple(t.shape), NAN, device=DEV) for t in (res, wf, st)]
    rmse = torch.full((1, b), NAN, device=DEV)
    eng.step_medium(wf, res, st, k_sq.to(DEV), None if k_im is None else k_im.to(DEV), q.to(DEV), src.to(DEV), 1, hist[0], hist[1], hist[2], rmse)
    torch.cuda.synchronize()
    eng.check_async_errors()
    w64, w32 = (_oracle_step(ti, k_sq, k_im, q, src, weights, h, w, dt) for dt in (torch.float64, torch.float32))
    report, ok = [], []
    for k, t in (("wf", wf), ("res", res)):
        ok.append(_vs_float64(k, t, w64[k], w32[k], report))
    o = 0
    for d in range(4):
        lv = slice(o, o + (h >> d) * (w >> d))
        o = lv.stop
        ok.append(_vs_float64(f"state{d}", st[:, :, lv], w64["states"][:, :, lv], w32["states"][:, :, lv], report))
    print(f"DENSITY step {h}x{w}x{b} lossy={lossy}: " + "; ".join(report))
    assert all(ok), report
    # the constant-density residual of the same wavefield is far from it: the plane is not ignored
    const = w64["res"] + DC.density_term(w64["wf"], q.double(), R.tables(h, w))
    assert float((res.cpu().double() - w64["res"]).abs().max()) < 0.01 * float((const - w64["res"]).abs().max())
    want = eng.rmse(res)
    assert float(((rmse[0] - want).abs() / want).max()) <= 1e-5, (rmse.tolist(), want.tolist())
    assert torch.equal(hist[0][0], res) and torch.equal(hist[1][0], wf) and torch.equal(hist[2][0], st)


# ------------------------------------------------------------------------------------------------------------------------------ 3: free run
def test_free_run_follows_the_oracle_and_converges(eng, weights):
    n, b, loc = 96, 2, [24, 48]
    sos, rho, q = DC.ring_medium(n)
    _, tr32 = DC.oracle_loop(n, sos, q, 20, weights, torch.float32, loc)
    eng.set_domain(n, *R.DOMAIN)
    k_sq, qd = ((1.0 / sos) ** 2).contiguous().to(DEV), q.to(DEV)
    src = R.point_source_map(n, n, loc, 10.0).to(DEV)

    def run(chunks):
        wf = torch.zeros(b, 2, n, n, device=DEV)
        res = eng.residual_medium(wf, k_sq, None, qd, src)
        st = torch.zeros(b, 2, eng.state_len, device=DEV)
        rows = []
        for k in chunks:
            rmse = torch.full((k, b), NAN, device=DEV)
            eng.step_medium(wf, res, st, k_sq, None, qd, src, k, rmse_hist=rmse)
            rows.append(rmse)
        torch.cuda.synchronize()
        eng.check_async_errors()
        return wf, res, st, torch.cat(rows)

    wf, res, st, rmse = run([300])
    rel = ((rmse[:20].cpu().double() - tr32.double()).abs() / tr32.double()).max().item()
    rows = {k: [f"{v:.2e}" for v in rmse[k - 1].tolist()] for k in (10, 50, 100, 200, 300)}
    print(f"DENSITY free run 96^2 (max|q| {float(q.abs().max()):.3f}): first 20 RMSE rows vs the fp32 oracle {rel:.2e}; "
          f"RMSE at 10 / 50 / 100 / 200 / 300: {rows}")
    assert rel <= 0.02
    assert bool((rmse[-1] <= 1.3e-3).all()), rmse[-1].tolist()
    true = eng.rmse(eng.residual_medium(wf, k_sq, None, qd, src))
    assert float(((true - rmse[-1]).abs() / true).max()) <= 1e-5
    # 300 iterations in one call equal 100 + 200 in two
    wf2, res2, st2, rmse2 = run([100, 200])
    assert torch.equal(wf, wf2) and torch.equal(res, res2) and torch.equal(st, st2)
    assert torch.allclose(rmse, rmse2, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------------------- 4: GMRES against the direct solve
@pytest.mark.parametrize("n,loc", [(32, [12, 16]), (48, [14, 24])])
def test_medium_gmres_vs_float64_direct_solve(n, loc):
    from helmnet_amd.gmres import gmres
    s = _solver(n, loc)
    sos, rho, q = DC.ring_medium(n)
    out = gmres(s, sos.to(DEV), restart=40, max_outer=200, tol=2e-6, backend="hip", density=rho.to(DEV))
    got = out["wavefield"].cpu().numpy()
    src = s.source.detach().cpu().numpy()[0]
    k_sq = ((1.0 / sos) ** 2).contiguous()
    print("iterations per sample", out["iterations_per_sample"].tolist(), "converged", out["converged"], "cycles", out["cycles"])
    assert out["converged"]
    for b in range(2):
        want, _ = DC.direct_solve(k_sq[b, 0].numpy(), None, q[b].numpy(), src)
        const = O.direct_solve(sos[b, 0].numpy(), src, *R.DOMAIN)
        err, scale = np.abs(got[b] - want).max(), np.abs(want).max()
        print(f"DENSITY gmres n={n} sample {b}: max|got - want| = {err:.3e}, bar {2e-4 * scale:.3e} (error / bar {err / (2e-4 * scale):.3f}); "
              f"the constant-density solution is {np.abs(const - want).max():.3f} away")
        assert err <= 2e-4 * scale, (b, err, scale)
    s.engine().check_async_errors()


# --------------------------------------------------------------------------------------------------------------------- 5: the flexible cycle
def _cycle_buffers(b, n, restart):
    return (torch.full((b, restart + 1, 2 * n * n), NAN, device=DEV), torch.full((b, restart, 2 * n * n), NAN, device=DEV),
            torch.full((b, restart + 1, restart, 2), NAN, device=DEV))


@pytest.mark.parametrize("lossy", [False, True])
def test_z_is_the_public_step_medium_composed_as_the_header_says(lossy):
    from helmnet_amd.gmres import default_precond_scale
    n, restart, m, b = 48, 4, 3, 2
    s = _solver(n, [14, 24])
    eng = s.engine()
    sos, rho, q = DC.ring_medium(n)
    k_sq, qd = ((1.0 / sos) ** 2).contiguous().to(DEV), q.to(DEV)
    k_im = (0.04 * (1.0 / sos)).contiguous().to(DEV) if lossy else None
    rhs = s.source.detach().float().contiguous()
    alpha = float(np.float32(default_precond_scale(rhs)))
    basis, zbasis, hess = _cycle_buffers(b, n, restart)
    x = torch.zeros(b, 2, n, n, device=DEV)
    rmse, k_used = eng.fgmres_cycle_medium(x, k_sq, k_im, qd, rhs, restart, 0.0, m, alpha, basis, hess, zbasis)
    torch.cuda.synchronize()
    eng.check_async_errors()
    assert bool(torch.isfinite(zbasis).all()) and k_used.tolist() == [restart] * b
    a = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    for j in range(restart):
        src = (a * basis[:, j]).reshape(b, 2, n, n).contiguous()
        wf = torch.zeros_like(src)
        res = torch.zeros_like(src) - src
        st = torch.zeros(b, 2, eng.state_len, device=DEV)
        eng.step_medium(wf, res, st, k_sq, k_im, qd, src, m)
        want = (wf / a).reshape(b, 2 * n * n)
        assert torch.equal(zbasis[:, j], want), j
        assert float(want.abs().max()) > 0.0
    # row 0 of rmse is the true residual of the start iterate under A_rho
    true0 = eng.rmse(eng.residual_medium(torch.zeros_like(x), k_sq, k_im, qd, rhs))
    assert torch.allclose(rmse[0], true0, rtol=1e-5, atol=0)
    # precond_iters = 0: plain restarted GMRES, zbasis == basis bit for bit; two calls on equal inputs give equal bits
    runs = []
    for _ in range(2):
        bs, zb, hs = _cycle_buffers(b, n, restart)
        x0 = torch.zeros(b, 2, n, n, device=DEV)
        r0, ku = eng.fgmres_cycle_medium(x0, k_sq, k_im, qd, rhs, restart, 0.0, 0, 1.0, bs, hs, zb)
        torch.cuda.synchronize()
        assert torch.equal(zb, bs[:, :restart])
        runs.append((x0, bs, hs, r0.clone(), ku.clone()))
    assert all(torch.equal(p, q_) for p, q_ in zip(*runs))
    eng.check_async_errors()


def test_learned_preconditioner_on_a_variable_density_medium():
    n = 96
    s = _solver(n, [24, 48])
    sos, rho, q = DC.ring_medium(n)
    sos, rho = sos.to(DEV), rho.to(DEV)
    pre = s.gmres(sos, restart=40, max_cycles=400, tol=2e-6, density=rho, precondition="learned")
    plain = s.gmres(sos, restart=40, max_cycles=400, tol=2e-6, density=rho)
    print(f"DENSITY gmres 96^2: learned {pre['cycles']} cycles ({pre['unet_evaluations']} UNet evaluations), plain {plain['cycles']} cycles")
    assert pre["converged"] and plain["converged"]
    assert pre["unet_evaluations"] == pre["cycles"] * 40 * 10 and plain["unet_evaluations"] == 0
    a, b = pre["wavefield"], plain["wavefield"]
    scale = float(b.abs().max())
    print(f"   max |learned - plain| = {float((a - b).abs().max()):.3e}, bar {4e-4 * scale:.3e}")
    assert float((a - b).abs().max()) <= 4e-4 * scale
    s.engine().check_async_errors()


# ------------------------------------------------------------------------------------------------------------------------------ 6: contract
def _raw_args(hw, b=2, restart=3):
    h, w = hw
    P = h * w
    new = lambda *shape: torch.full(shape, NAN, device=DEV)  # noqa: E731
    ti = R.teacher_inputs(h, w, b, 43)
    g = {k: v.to(DEV) for k, v in ti.items()}
    alpha = (0.1 * (g["sos"] - 1.0)).contiguous()
    k = 1.0 / g["sos"]
    return dict(wf=g["wf"], res=g["res"].clone(), st=g["states"], k_sq=(k ** 2 - alpha ** 2).contiguous(), k_im=(2.0 * k * alpha).contiguous(),
                rho=DC.seeded_q(h, w, b).to(DEV), src=R.point_source_map(h, w, [h // 4, w // 2], 10.0).to(DEV),
                out=new(b, 2, h, w), rmse_hist=new(1, b), basis=new(b, restart + 1, 2 * P), zbasis=new(b, restart, 2 * P), hess=new(b, restart + 1, restart, 2),
                rmse=new(restart + 1, b), k_used=torch.full((b,), -7, device=DEV, dtype=torch.int32))


def _residual(e, a, rho, out=None, k_im="given"):
    out = a["out"] if out is None else out
    k_im = a["k_im"] if isinstance(k_im, str) else k_im
    return e.lib.hn_residual_medium(e.ctx, _ptr(a["wf"]), _ptr(a["k_sq"]), _ptr(k_im), _ptr(rho), _ptr(a["src"]), 1, _ptr(out), a["wf"].shape[0], e._stream())


def _step(e, a, rho, wf, res, st):
    return e.lib.hn_step_medium(e.ctx, _ptr(wf), _ptr(res), _ptr(st), _ptr(a["k_sq"]), _ptr(a["k_im"]), _ptr(rho), _ptr(a["src"]), 1, wf.shape[0], 1, None, None,
                                None, _ptr(a["rmse_hist"]), e._stream())


def _cycle(e, a, rho, x, iters=0):
    return e.lib.hn_fgmres_cycle_medium(e.ctx, _ptr(x), _ptr(a["k_sq"]), _ptr(a["k_im"]), _ptr(rho), _ptr(a["src"]), 1, x.shape[0], 3, 0.0, iters, 1.0,
                                        _ptr(a["basis"]), _ptr(a["zbasis"]), _ptr(a["hess"]), _ptr(a["rmse"]), _ptr(a["k_used"]), e._stream())


OUTPUTS = ("out", "rmse_hist", "basis", "zbasis", "hess", "rmse", "k_used")


def _untouched(a):
    torch.cuda.synchronize()
    for k in OUTPUTS:
        t = a[k]
        assert bool((t == -7).all()) if t.dtype == torch.int32 else bool(torch.isnan(t).all()), k


def _off4(t):
    """A copy of ``t`` whose first element lies 4 bytes behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1: 1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


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

        # rho_grad = NULL: HN_ERR_ARG naming the constant-density siblings
        for call, lossy, lossless in ((lambda: _residual(e, a, None), "hn_residual_lossy", "hn_residual"), (lambda: _step(e, a, None, wf, res, st), "hn_step_lossy", "hn_step"),
                                      (lambda: _cycle(e, a, None, wf), "hn_fgmres_cycle_lossy", "hn_fgmres_cycle")):
            assert call() == ERR_ARG
            assert "rho_grad is NULL" in _err(e) and lossy + "," in _err(e) and " " + lossless + " " in _err(e), _err(e)
        _untouched(a)
        inputs_unchanged()
        # a rho_grad that overlaps res (the last plane of res is the first of rho_grad); for the cycle, one that lies in the basis, and k_sq_im itself
        P = n * n
        buf = torch.full((8 * P,), NAN, device=DEV)
        res_v, rho_v = buf[: 4 * P].view(2, 2, n, n), buf[3 * P: 7 * P].view(2, 2, n, n)
        assert _residual(e, a, rho_v, out=res_v) == ERR_ARG and "rho_grad overlaps res" in _err(e), _err(e)
        assert _step(e, a, rho_v, wf, res_v, st) == ERR_ARG and "overlaps" in _err(e) and "rho_grad" in _err(e), _err(e)
        assert _cycle(e, a, a["basis"].view(-1)[: 4 * P].view(2, 2, n, n), wf) == ERR_ARG and "rho_grad overlaps basis" in _err(e), _err(e)
        both = torch.zeros(4 * P, device=DEV)
        a2 = dict(a, k_im=both[: 2 * P].view(2, 1, n, n))
        assert _cycle(e, a2, both.view(2, 2, n, n), wf) == ERR_ARG and "k_sq_im overlaps rho_grad" in _err(e), _err(e)
        # the cycle reads its fields as float4: a rho_grad that is only 4-byte aligned is refused
        assert _cycle(e, a, _off4(a["rho"]), wf) == ERR_ARG and "rho_grad is not 16-byte aligned" in _err(e), _err(e)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf).all())
        _untouched(a)
        inputs_unchanged()
        # the first call on a square domain under capture: HN_ERR_STATE, nothing enqueued
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = _residual(e, a, a["rho"])
        torch.cuda.synchronize()
        assert rc == ERR_STATE and "capture" in _err(e), (rc, _err(e))
        _untouched(a)
        # ... and after an eager call the same call is captured and replayed
        eager = e.residual_medium(a["wf"], a["k_sq"], a["k_im"], a["rho"], a["src"])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = _residual(e, a, a["rho"])
            assert rc == OK, _err(e)
            graph.replay()
            torch.cuda.synchronize()
        assert torch.equal(a["out"], eager)
        a["out"].fill_(NAN)
        # the residual and the step take buffers that are only 4-byte aligned: the same bits
        m = dict(a, wf=_off4(a["wf"]), k_sq=_off4(a["k_sq"]), k_im=_off4(a["k_im"]), src=_off4(a["src"]))
        out4 = _off4(a["out"])
        assert _residual(e, m, _off4(a["rho"]), out=out4) == OK, _err(e)
        torch.cuda.synchronize()
        assert torch.equal(out4, eager)
        assert _residual(e, m, _off4(a["rho"]), out=out4, k_im=None) == OK, _err(e)
        torch.cuda.synchronize()
        assert torch.equal(out4, e.residual_medium(a["wf"], a["k_sq"], None, a["rho"], a["src"]))
        runs = []
        for rho, kim in ((a["rho"], a["k_im"]), (_off4(a["rho"]), _off4(a["k_im"]))):
            w1, r1, s1 = a["wf"].clone(), a["res"].clone(), a["st"].clone()
            assert _step(e, dict(a, k_im=kim), rho, w1, r1, s1) == OK, _err(e)
            torch.cuda.synchronize()
            runs.append((w1, r1, s1))
        assert all(torch.equal(p, q) for p, q in zip(*runs))
        a["rmse_hist"].fill_(NAN)
        e.check_async_errors()
        # HN_OPT_LANES 2
        e.set_option("lanes", 2)
        assert _step(e, a, a["rho"], wf, res, st) == ERR_UNSUPPORTED and "HN_OPT_LANES" in _err(e), _err(e)
        e.set_option("lanes", 1)
        _untouched(a)
        inputs_unchanged()
        # the cycle on a rectangular domain
        e.set_domain_rect(32, 80, *R.DOMAIN)
        r = _raw_args((32, 80))
        x = r["wf"].clone()
        assert _cycle(e, r, r["rho"], x) == ERR_UNSUPPORTED and "rectangular domain" in _err(e) and "32 x 80" in _err(e), _err(e)
        _untouched(r)
        assert torch.equal(x, r["wf"])
    finally:
        e.close()


def _existing(e, n, b=2):
    """hn_residual, hn_residual_lossy and two hn_step iterations on seeded inputs."""
    ti = R.teacher_inputs(n, n, b, 300 + n)
    g = {k: v.to(DEV) for k, v in ti.items()}
    k_sq = ((1.0 / g["sos"]) ** 2).contiguous()
    k_im = LC.seeded_k_sq_im(n, n, b, 77).to(DEV)
    src = R.point_source_map(n, n, [n // 4, n // 2], 10.0).to(DEV)
    res0 = e.residual(g["wf"], k_sq, src)
    lres = e.residual_lossy(g["wf"], k_sq, k_im, src)
    wf, res, st = g["wf"].clone(), res0.clone(), g["states"].clone()
    hist = [torch.full((2,) + tuple(t.shape), NAN, device=DEV) for t in (res, wf, st)]
    rmse = torch.full((2, b), NAN, device=DEV)
    e.step(wf, res, st, k_sq, src, 2, hist[0], hist[1], hist[2], rmse)
    torch.cuda.synchronize()
    e.check_async_errors()
    return [res0, wf, res, st, rmse, lres] + hist


@pytest.mark.parametrize("n", [96, 144])
def test_medium_calls_leave_the_existing_entry_points_alone(blob, n):
    e, fresh = _engine(blob=blob), _engine(blob=blob)
    try:
        for x in (e, fresh):
            x.set_domain(n, *R.DOMAIN)
        route = e.counter("spectral_route")
        before = _existing(fresh, n)      # an engine that never makes a medium call; on `e` the medium calls come first and build the line tables
        a = _raw_args((n, n))
        e.residual_medium(a["wf"], a["k_sq"], a["k_im"], a["rho"], a["src"])
        e.residual_medium(a["wf"], a["k_sq"], None, a["rho"], a["src"])
        wf, res, st = a["wf"].clone(), a["res"].clone(), a["st"].clone()
        e.step_medium(wf, res, st, a["k_sq"], a["k_im"], a["rho"], a["src"], 2)
        x = a["wf"].clone()
        e.fgmres_cycle_medium(x, a["k_sq"], a["k_im"], a["rho"], a["src"], 3, 0.0, 1, 1.0)
        torch.cuda.synchronize()
        e.check_async_errors()
        assert e.counter("spectral_route") == route
        for i, (p, q) in enumerate(zip(_existing(e, n), before)):
            assert not bool(torch.isnan(p).any())
            if i == 4:      # the RMSE rows: one atomicAdd per block
                assert torch.allclose(p, q, rtol=1e-5, atol=0)
            else:
                assert torch.equal(p, q), i
    finally:
        e.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------------------------------ 7: Python front end
def test_python_front_end():
    n = 96
    s = _solver(n, [24, 48])
    sos, rho, q = DC.ring_medium(n)
    sos, rho, q = sos.to(DEV), rho.to(DEV), q.to(DEV)
    alpha = LC.ring_alpha(sos, 0.02)
    # density=None: the code path and the bits of before
    x, y = s.forward(sos, num_iterations=3), s.forward(sos, num_iterations=3, density=None)
    assert all(torch.equal(p, r) for k in ("wavefields", "residuals") for p, r in zip(x[k], y[k]))
    out = s.forward(sos, num_iterations=3, return_wavefields=True, return_states=True, density=rho)
    assert set(out) == set(s.forward(sos, num_iterations=3, return_wavefields=True, return_states=True)) and out["last_iteration"] == 2
    assert all(tuple(t.shape) == (2, 2, n, n) for t in out["wavefields"] + out["residuals"]) and len(out["wavefields"]) == len(out["residuals"]) == 3
    assert tuple(out["states"][0].shape) == (2, 2, R.state_len(n, n)) and tuple(out["residual_norms"].shape) == (3, 2)
    assert not torch.equal(out["wavefields"][-1], x["wavefields"][-1])
    # the front end's gradient is the tests' restatement to fp32 rounding, and get_residual(rho_grad=) is the loop's residual
    from helmnet_amd.density import log_density_gradient
    front = log_density_gradient(rho)
    assert float((front - q).abs().max()) <= 1e-7
    k_sq = ((1.0 / sos) ** 2).contiguous()
    assert torch.equal(s.get_residual(out["wavefields"][-1], k_sq, rho_grad=front), out["residuals"][-1])
    # a map that is constant per sample broadcasts, and is the constant-density medium to fp32 rounding
    flat = s.forward(sos, num_iterations=2, density=torch.full((1, 1, 1, 1), 1000.0, device=DEV), residuals="last")
    const = s.forward(sos, num_iterations=2, residuals="last")
    assert float((flat["wavefields"][0] - const["wavefields"][0]).abs().max()) <= 1e-4 * float(const["wavefields"][0].abs().max())
    # with absorption: both planes and the density term
    both = s.forward(sos, num_iterations=3, absorption=alpha, density=rho, residuals="last")
    k_re, k_im = (1.0 / sos) ** 2 - alpha ** 2, 2.0 * (1.0 / sos) * alpha
    assert torch.equal(s.get_residual(both["wavefields"][0], k_re.contiguous(), k_im.contiguous(), front), both["residuals"][0])
    assert not torch.equal(both["wavefields"][0], out["wavefields"][-1])
    cont = s.n_steps(out["wavefields"][0], k_sq, out["residuals"][0], 2, density=rho, residuals="last")
    assert tuple(cont["wavefields"][0].shape) == (2, 2, n, n)
    tol = s.solve_to_tolerance(sos, 2e-3, max_iterations=600, density=rho)
    print(f"DENSITY python: solve_to_tolerance(2e-3) at 96^2: {tol['iterations']} iterations, converged {tol['converged']}, "
          f"last rmse {tol['residual_norms'][-1].tolist()}")
    assert tol["converged"] and tol["iterations"] <= 600
    with pytest.raises(RuntimeError, match="grad"):
        s.forward(sos.clone().requires_grad_(True), num_iterations=2, density=rho)
    s.engine().check_async_errors()
