"""hn_fgmres_refine_cycle_lossy on the GPU: one refinement step against its own definition (hn_residual_f64_lossy, then hn_fgmres_cycle_lossy on
fp32(-res / s) from zero, then x + s d in float64), the per-sample stop, bit-reproducibility, the refusals, and the ground truth it exists for --
``gmres64(absorption=...)`` to 1e-10 against a float64 direct solve, and ``reference_error(absorption=...)``.  Needs a real MI355X.

Media are the ring problems of tests/lossy_adjoint_common.py (``LA.ring_problem``), the dense operator is ``LA.lossy_matrix`` and the CPU float64
residual ``LC.residual``: none of it comes from the code under test.

Ground-truth bar.  For M u* = b and a computed u with r = b - M u:  u - u* = -M^-1 r, so ||u - u*||_2 <= ||r||_2 / sigma_min(M); the test adds
1e-12 ||u*||_2 for the direct solve's own error (numpy's LU in float64 on a matrix whose condition number is a few hundred) and computes sigma_min
by SVD.  The residual norm itself is confirmed on the CPU to 1e-11 of max (the operator's bar, tests/test_f64_gpu.py)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import lossy_adjoint_common as LA
import lossy_common as LC
import rect_common as R
from oracle import helmnet_oracle as O

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3
RESTART = 8
_SOLVERS = {}


def _p(t):
    if t is None or isinstance(t, int):
        return t or None
    return ctypes.c_void_p(t.data_ptr())


def _solver(n):
    from helmnet_amd import IterativeSolver
    if n not in _SOLVERS:
        s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
        s.set_domain_size(n, source_location=[n // 2 - 2, n // 2])
        _SOLVERS[n] = s
    return _SOLVERS[n]


@pytest.fixture(autouse=True)
def _async_errors_clean():
    yield
    torch.cuda.synchronize()
    for s in _SOLVERS.values():
        s.engine().check_async_errors()


def _problem(n, batch, a0=0.1):
    """The solver, the fp32 planes it forms on the device from LA.ring_problem's (sos, alpha) -- the medium ``gmres64(absorption=...)`` solves, bit
    for bit -- and its source."""
    from helmnet_amd.absorption import complex_k_sq
    s = _solver(n)
    p = LA.ring_problem(n, a0, b=batch)
    k_sq, k_im = complex_k_sq(p["sos"].to(DEV), p["alpha"].to(DEV), s.hparams.omega)
    return s, k_sq.contiguous(), k_im.contiguous(), s.source.detach().float().contiguous()


def _alpha(rhs):
    from helmnet_amd.gmres import default_precond_scale
    return default_precond_scale(rhs)


def _refine(eng, k_sq, k_im, rhs, restart, tol, floor, m, alpha, x=None):
    b, n = k_sq.shape[0], k_sq.shape[-1]
    x = torch.zeros(b, 2, n, n, device=DEV, dtype=torch.float64) if x is None else x.clone()
    nan = float("nan")
    basis, zbasis = torch.full((b, restart + 1, 2 * n * n), nan, device=DEV), torch.full((b, restart, 2 * n * n), nan, device=DEV)
    hess = torch.full((b, restart + 1, restart, 2), nan, device=DEV)
    rmse64, rmse, k_used = eng.fgmres_refine_cycle_lossy(x, k_sq, k_im, rhs, restart, tol, m, alpha, floor, basis, hess, zbasis)
    return {"x": x, "basis": basis, "zbasis": zbasis, "hess": hess, "rmse": rmse, "k_used": k_used, "rmse64": rmse64}


_KEYS = ("x", "rmse64", "rmse", "k_used", "basis", "zbasis", "hess")


def _fused_or_two_step(x0, s, d):
    """x0 + s * d per element with ONE rounding (a fused multiply-add) and with two, exactly, by rational arithmetic on the host."""
    x0, d = x0.reshape(-1).tolist(), d.reshape(-1).tolist()
    fs = Fraction(s)
    fused = [float(Fraction(a) + fs * Fraction(b)) for a, b in zip(x0, d)]
    two = [a + s * b for a, b in zip(x0, d)]
    return torch.tensor(fused, dtype=torch.float64), torch.tensor(two, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------------ 1, 2, 3
@pytest.mark.parametrize("n,batch,m", [(48, 2, 0), (48, 2, 2), (96, 1, 0)])
def test_one_cycle_is_residual64_lossy_then_the_fp32_lossy_cycle_then_x_plus_s_d(n, batch, m):
    s, k_sq, k_im, rhs = _problem(n, batch)
    eng = s.engine()
    alpha, tol, floor = _alpha(rhs), 1e-10, 1e-6
    g = torch.Generator().manual_seed(900 + n + m)
    x0 = (0.05 * torch.randn(batch, 2, n, n, generator=g, dtype=torch.float64)).to(DEV)
    for start in (None, x0):
        run = _refine(eng, k_sq, k_im, rhs, RESTART, tol, floor, m, alpha, x=start)
        xs = torch.zeros_like(x0) if start is None else start
        res, want_rmse = eng.residual64_lossy(xs, k_sq.double(), k_im.double(), rhs.double(), True, True)
        assert torch.equal(run["rmse64"], want_rmse)                                        # 1: bit for bit
        sc = want_rmse.clamp_min(1e-300).reshape(batch, 1, 1, 1)
        rhs32 = (-res / sc).float().contiguous()
        d = torch.zeros(batch, 2, n, n, device=DEV)
        basis, zbasis, hess = (torch.full_like(run[k], float("nan")) for k in ("basis", "zbasis", "hess"))
        assert all(max(tol / float(r), floor) == floor for r in want_rmse.tolist())          # every sample's inner tolerance max(tol / s, floor) is the floor
        rmse, k_used = eng.fgmres_cycle_lossy(d, k_sq, k_im, rhs32, RESTART, floor, m, alpha, basis, hess, zbasis)
        print(f"n={n} m={m} from {'zero' if start is None else 'x0'}: rmse64 {want_rmse.tolist()}, inner row 0 {rmse[0].tolist()}, k_used {k_used.tolist()}")
        assert torch.equal(run["k_used"], k_used) and torch.equal(run["rmse"], rmse)        # 2
        assert torch.equal(run["basis"], basis) and torch.equal(run["zbasis"], zbasis) and torch.equal(run["hess"], hess)
        assert k_used.tolist() == [RESTART] * batch
        if m == 0:
            assert torch.equal(zbasis, basis[:, :RESTART])
        if start is None:
            assert torch.equal(run["x"], sc * d.double())                                   # 3: x = 0 + s d, one rounding however it is formed
        else:
            fused, two = _fused_or_two_step(xs[0].cpu(), float(sc[0]), d[0].double().cpu())
            got = run["x"][0].cpu().reshape(-1)
            assert torch.equal(got, fused) or torch.equal(got, two)                         # 3: x + s d formed in float64, with or without a fused multiply-add
            assert float((run["x"] - (xs + sc * d.double())).abs().max()) <= 2.0 ** -52 * float(run["x"].abs().max())


# ------------------------------------------------------------------------------------------------------------------ 4, 5
def test_a_sample_below_tol_and_a_sample_with_zero_residual_are_untouched():
    n = 48
    s, k_sq, k_im, rhs = _problem(n, 3)
    eng = s.engine()
    p = LA.ring_problem(n, 0.1, b=3)
    tol = 1e-10
    solved = s.gmres64(p["sos"][:1].to(DEV), restart=20, max_cycles=400, tol=tol, absorption=p["alpha"][:1].to(DEV))
    assert solved["converged"]
    x0 = torch.cat([solved["wavefield"], torch.zeros(2, 2, n, n, device=DEV, dtype=torch.float64)]).contiguous()
    # sample 1: the zero field against a zero right-hand side has a residual of exactly zero
    rhs3 = torch.cat([rhs, torch.zeros_like(rhs), rhs]).contiguous()
    run = _refine(eng, k_sq, k_im, rhs3, RESTART, tol, 1e-6, 0, 1.0, x=x0)
    print("rmse64", run["rmse64"].tolist(), "k_used", run["k_used"].tolist())
    assert 0.0 < float(run["rmse64"][0]) < tol and float(run["rmse64"][1]) == 0.0
    assert run["k_used"].tolist() == [0, 0, RESTART]
    assert torch.equal(run["x"][:2], x0[:2]) and not torch.equal(run["x"][2], x0[2])
    # the third sample's bits do not depend on its batch mates
    one = _refine(eng, k_sq[2:].contiguous(), k_im[2:].contiguous(), rhs, RESTART, tol, 1e-6, 0, 1.0)
    for key in ("x", "basis", "zbasis", "hess", "k_used", "rmse64"):
        assert torch.equal(one[key][0], run[key][2]), key
    assert torch.equal(one["rmse"][:, 0], run["rmse"][:, 2])


@pytest.mark.parametrize("m", [0, 2])
def test_two_calls_give_equal_bits_and_a_samples_bits_do_not_depend_on_its_batch(m):
    n = 48
    s, k_sq, k_im, rhs = _problem(n, 2)
    eng = s.engine()
    alpha = _alpha(rhs)
    a = _refine(eng, k_sq, k_im, rhs, RESTART, 1e-10, 1e-6, m, alpha)
    b = _refine(eng, k_sq, k_im, rhs, RESTART, 1e-10, 1e-6, m, alpha)
    for key in _KEYS:
        assert torch.equal(a[key], b[key]), key
    one = _refine(eng, k_sq[1:].contiguous(), k_im[1:].contiguous(), rhs, RESTART, 1e-10, 1e-6, m, alpha)
    for key in ("x", "basis", "zbasis", "hess", "k_used", "rmse64"):
        assert torch.equal(one[key][0], a[key][1]), key
    assert torch.equal(one["rmse"][:, 0], a["rmse"][:, 1])


# ------------------------------------------------------------------------------------------------------------------ 6: refusals
def _raw(eng, x, k_sq, k_sq_im, rhs, rhs_batch, batch, restart, tol, floor, m, alpha, basis, zbasis, hess, rmse, k_used, rmse64):
    return eng.lib.hn_fgmres_refine_cycle_lossy(eng.ctx, _p(x), _p(k_sq), _p(k_sq_im), _p(rhs), rhs_batch, batch, restart, tol, floor, m, alpha, _p(basis),
                                                _p(zbasis), _p(hess), _p(rmse), _p(k_used), _p(rmse64), eng._stream())


def _buffers(h, w, batch, restart):
    f = lambda *shape: torch.full(shape, -7.0, device=DEV)  # noqa: E731
    return dict(x=torch.zeros(batch, 2, h, w, device=DEV, dtype=torch.float64), basis=f(batch, restart + 1, 2 * h * w), zbasis=f(batch, restart, 2 * h * w),
                hess=f(batch, restart + 1, restart, 2), rmse=f(restart + 1, batch), k_used=torch.full((batch,), -7, device=DEV, dtype=torch.int32),
                rmse64=torch.full((batch,), -7.0, device=DEV, dtype=torch.float64))


def _left_alone(bufs):
    torch.cuda.synchronize()
    assert float(bufs["x"].abs().max()) == 0.0
    for k, t in bufs.items():
        assert k == "x" or bool((t == -7).all()), k


def test_argument_refusals_leave_the_outputs_alone():
    n, batch, restart = 48, 2, 4
    s, k_sq, k_im, rhs = _problem(n, batch)
    eng = s.engine()
    bufs = _buffers(n, n, batch, restart)
    err = lambda: eng.lib.hn_last_error(eng.ctx).decode()  # noqa: E731
    call = lambda **kw: _raw(eng, **{**dict(k_sq=k_sq, k_sq_im=k_im, rhs=rhs, rhs_batch=1, batch=batch, restart=restart, tol=1e-10, floor=1e-6, m=1,  # noqa: E731
                                            alpha=1.0, **bufs), **kw})
    assert call(k_sq_im=0) == ERR_ARG and "k_sq_im is NULL" in err() and "hn_fgmres_refine_cycle)" in err()      # names the lossless sibling
    assert call(k_sq_im=k_im.data_ptr() + 4) == ERR_ARG and "k_sq_im is not 16-byte aligned" in err()
    assert call(k_sq_im=k_sq) == ERR_ARG and "overlaps" in err() and "k_sq_im" in err()
    assert call(k_sq_im=bufs["basis"]) == ERR_ARG and "overlaps" in err() and "k_sq_im" in err()
    as_f32 = bufs["x"].view(torch.float32).reshape(-1)
    assert call(k_sq_im=as_f32[as_f32.numel() // 2:]) == ERR_ARG and "k_sq_im overlaps x" in err()               # the second half of the float64 x
    # the sibling's own
    assert call(tol=float("nan")) == ERR_ARG and "tol" in err()
    assert call(floor=-1.0) == ERR_ARG and "inner_floor" in err()
    assert call(m=-2) == ERR_ARG and "precond_iters" in err()
    assert call(alpha=float("inf")) == ERR_ARG and "precond_scale" in err()
    assert call(zbasis=0) == ERR_ARG and "NULL" in err()
    assert call(rmse64=0) == ERR_ARG and "NULL" in err()
    assert call(restart=65) == ERR_ARG and "restart" in err()
    assert call(rhs_batch=3) == ERR_ARG and "rhs batch" in err()
    _left_alone(bufs)
    with pytest.raises(RuntimeError, match="grad"):
        eng.fgmres_refine_cycle_lossy(bufs["x"], k_sq, k_im.clone().requires_grad_(True), rhs, restart, 1e-10, 0, 1.0)


def test_a_rectangle_is_unsupported_and_capture_is_refused():
    from helmnet_amd.engine import Engine
    eng = Engine(torch.device(DEV))
    try:
        h, w, batch, restart = 32, 80, 1, 3
        eng.set_domain_rect(h, w, *R.DOMAIN)
        bufs = _buffers(h, w, batch, restart)
        k_sq, k_im, rhs = torch.ones(batch, 1, h, w, device=DEV), torch.full((batch, 1, h, w), 0.1, device=DEV), torch.ones(1, 2, h, w, device=DEV)
        args = dict(k_sq=k_sq, k_sq_im=k_im, rhs=rhs, rhs_batch=1, batch=batch, restart=restart, tol=1e-10, floor=1e-6, m=0, alpha=1.0)
        assert _raw(eng, **args, **bufs) == ERR_UNSUPPORTED
        assert "rectangular" in eng.lib.hn_last_error(eng.ctx).decode()
        _left_alone(bufs)
        n = 48
        eng.set_domain(n, *R.DOMAIN)
        bufs = _buffers(n, n, batch, restart)
        p = LA.ring_problem(n, 0.1, b=1)
        args.update(k_sq=p["k_sq"].to(DEV), k_sq_im=p["k_sq_im"].to(DEV), rhs=torch.ones(1, 2, n, n, device=DEV))
        probe = torch.zeros(4, device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            probe.add_(1.0)
            rc = _raw(eng, **args, **bufs)
            msg = eng.lib.hn_last_error(eng.ctx).decode()
        assert rc == ERR_STATE and "captur" in msg
        g.replay()                                     # the capture is still valid, and holds nothing of the library's
        torch.cuda.synchronize()
        assert probe.tolist() == [1.0] * 4
        _left_alone(bufs)
        assert _raw(eng, **args, **bufs) == OK         # eager, without the network (precond_iters 0)
        torch.cuda.synchronize()
        assert bufs["k_used"].tolist() == [restart] and float(bufs["rmse64"][0]) > 0
        eng.check_async_errors()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 7: ground truth
_SIGMA_MIN = {}


def _direct(n, a0, b, k_sq, k_sq_im, src):
    """(u*, sigma_min(M)) of sample b of LA.ring_problem(n, a0), given as the fp32 planes the device holds: numpy's float64 direct solve and SVD of
    LA.lossy_matrix, once."""
    key = (n, a0, b)
    if key not in _SIGMA_MIN:
        M = LA.lossy_matrix(k_sq[b, 0].numpy(), k_sq_im[b, 0].numpy())
        _SIGMA_MIN[key] = (np.linalg.solve(M, src), float(np.linalg.svd(M, compute_uv=False)[-1]))
    return _SIGMA_MIN[key]


@pytest.mark.parametrize("a0", [0.02, 0.1])
@pytest.mark.parametrize("precondition", [None, "learned"])
def test_gmres64_with_absorption_reaches_the_direct_solve(a0, precondition):
    from helmnet_amd.absorption import complex_k_sq
    n, tol = 48, 1e-10
    s = _solver(n)
    p = LA.ring_problem(n, a0, b=2)
    sos, alpha = p["sos"].to(DEV), p["alpha"].to(DEV)
    out = s.gmres64(sos, restart=20, max_cycles=400, tol=tol, absorption=alpha, precondition=precondition)
    x = out["wavefield"]
    print(f"a0={a0} {precondition}: cycles {out['cycles']}, inner iterations {out['iterations_per_sample'].tolist()}, residual_norm64 "
          f"{out['residual_norm64'].tolist()}, unet evaluations {out['unet_evaluations']}")
    assert out["converged"] and x.dtype == torch.float64 and float(out["residual_norm64"].max()) < tol
    assert torch.equal(out["residual_norms"][-1], out["residual_norm64"])
    assert sorted(out) == sorted(s.gmres64(sos, restart=4, max_cycles=1, tol=tol))                  # the lossless dictionary's keys
    # the fp32 planes the solver formed from (sos, alpha) on the device, and its source
    k_sq, k_im = (t.cpu() for t in complex_k_sq(sos, alpha, s.hparams.omega))
    src = s.source.detach().float().cpu()
    t64 = R.tables(n, n)
    res = LC.residual(x.cpu(), k_sq.double(), k_im.double(), src.double(), t64)
    rmse_cpu = res.pow(2).mean((1, 2, 3)).sqrt()
    # The CPU residual confirms residual_norm64.  The residual is a difference of terms of size `scale`; either evaluation is within 1e-11 * scale
    # of the truth (the operator's bar), which at n = 48 leaves room: by the same derivation (a sum of n products, rounding n * 2^-53 of the largest
    # term, a factor of 50) each is within 50 * n * 2^-53 * scale, and the two norms differ by at most twice that.
    scale = max(float(O.apply_laplacian(x.cpu(), t64).abs().max()), float(LC.complex_term(x.cpu(), k_sq.double(), k_im.double()).abs().max()),
                float(src.abs().max()))
    d_norm = float((rmse_cpu - out["residual_norm64"].cpu()).abs().max())
    print(f"  CPU float64 residual norm {rmse_cpu.tolist()}: differs by {d_norm:.3e}; 1e-11 * scale {1e-11 * scale:.3e}, derived {100 * n * 2.0 ** -53 * scale:.3e}")
    assert d_norm <= 1e-11 * scale and d_norm <= 100 * n * 2.0 ** -53 * scale, (rmse_cpu.tolist(), out["residual_norm64"].tolist())
    bvec = (src[0, 0].double() + 1j * src[0, 1].double()).reshape(-1).numpy()
    for b in range(2):
        want, smin = _direct(n, a0, b, k_sq, k_im, bvec)
        got = (x[b, 0] + 1j * x[b, 1]).reshape(-1).cpu().numpy()
        r = (res[b, 0] + 1j * res[b, 1]).reshape(-1).numpy()
        err, bound = np.linalg.norm(got - want), np.linalg.norm(r) / smin + 1e-12 * np.linalg.norm(want)
        print(f"  sample {b}: |u - u*|_2 {err:.3e} <= |r|_2 / sigma_min + 1e-12 |u*|_2 = {bound:.3e} (sigma_min {smin:.4f}, |u*|_2 {np.linalg.norm(want):.3e})")
        assert err <= bound, (b, err, bound)


# ------------------------------------------------------------------------------------------------------------------ 8: reference_error
def test_reference_error_with_absorption_at_96():
    n = 96
    s = _solver(n)
    p = LA.ring_problem(n, 0.1, b=2)
    sos, alpha = p["sos"].to(DEV), p["alpha"].to(DEV)
    wf = s.forward(sos, num_iterations=100, absorption=alpha)["wavefields"][0]
    before = wf.clone()
    out = s.reference_error(wf, sos, absorption=alpha)
    lossless = s.reference_error(wf, sos, max_cycles=1)
    print(f"reference_error(absorption) at {n}: linf {out['linf'].tolist()}, rms {out['rms'].tolist()}, reference rmse64 {out['reference_rmse64'].tolist()}, "
          f"cycles {out['cycles']}")
    assert out["converged"] and float(out["reference_rmse64"].max()) < 1e-10
    assert sorted(out) == sorted(lossless) == ["converged", "cycles", "linf", "reference", "reference_rmse64", "rms"]
    assert torch.equal(wf, before) and out["reference"].dtype == torch.float64
    diff = wf.double() - out["reference"]
    assert torch.equal(out["linf"], diff.abs().amax((1, 2, 3))) and torch.equal(out["rms"], diff.pow(2).mean((1, 2, 3)).sqrt())
    assert float(out["linf"].min()) > 0.0                 # the learned iterate is not the ground truth
    # the reference solves the LOSSY problem: its float64 lossy residual is the reported one
    from helmnet_amd.absorption import complex_k_sq
    k_sq, k_im = complex_k_sq(sos, alpha, s.hparams.omega)
    norm = s.engine().residual64_lossy(out["reference"], k_sq.double(), k_im.double(), s.source.detach().double().contiguous(), False, True)[1]
    assert torch.equal(norm, out["reference_rmse64"])
