"""The adjoint of the variable-density operator and its adjoint-state gradients on the GPU: hn_residual_vjp_medium, hn_fgmres_adjoint_cycle_medium,
hn_adjoint_grad_medium, ``gmres_adjoint(density=)`` and ``IterativeSolver.solve_implicit(density=)`` against the float64 references composed in
tests/density_adjoint_common.py.  Needs a real MI355X.  Every figure is printed beside its bar before it is asserted (pytest -s).

Bars:
    operator        ``lossy_adjoint_common.adjoint_case``'s bar (without k_sq_im: its lossless bar) plus SP.BAR * density_share(g, q, t), the way
                    ``density_common.forward_case`` widens the forward bar; with q = 0 twice the constant-density bar against hn_residual_vjp_lossy
                    (hn_residual_vjp): two fp32 routes, each within one bar of float64
    inner product   |<A_rho u, g> - <u, A_rho^H g>| <= 1e-5 * max(|<A_rho u, g>|, 1), summed in float64
    dJ/dq           max|lam| * (SP.BAR * density_share(u, 1, t) + 4e-7 * max|b D u|): the first-derivative pass at the forward operator's bar for the
                    same term, then a two-term fp32 product sum (test_lossy_adjoint_gpu's pointwise bar)
    one cycle       4 x what hn_fgmres_cycle_medium shows for the same invariant on the forward system with the same planes, rhs and settings
    adjoint solve   max|lam - lam64| <= 2e-4 * max|lam64| against solve(M^H, g) in float64
    gradients       4e-4 * max|lam| * max|u| times the chain factors of ``density_adjoint_common.gradient_reference``
"""
import ctypes

import numpy as np
import pytest
import torch

import density_adjoint_common as DA
import density_common as DC
import lossy_adjoint_common as LA
import lossy_common as LC
import rect_common as R
import spectral_probes as SP
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3
NAN = float("nan")
_SOLVERS = {}


def _p(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _err(e):
    return e.lib.hn_last_error(e.ctx).decode()


@pytest.fixture(scope="module")
def blob(weights_np):
    from helmnet_amd.engine import pack_weights
    return pack_weights(weights_np, 4, "prelu")


def _engine(blob=None):
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    if blob is not None:
        e.load_weights(blob, 8, 4, 2, "prelu")
    return e


@pytest.fixture(scope="module")
def eng(blob):
    e = _engine(blob)
    yield e
    e.close()


def _solver(n, loc):
    from helmnet_amd import IterativeSolver
    key = (n, loc[0], loc[1])
    if key not in _SOLVERS:
        s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
        s.set_domain_size(n, source_location=list(loc))
        _SOLVERS[key] = s
    return _SOLVERS[key]


@pytest.fixture(autouse=True)
def _async_errors_clean():
    yield
    torch.cuda.synchronize()
    for s in _SOLVERS.values():
        s.engine().check_async_errors()


def _alpha_scale(src):
    from helmnet_amd.gmres import default_precond_scale
    return float(np.float32(default_precond_scale(src)))


# ------------------------------------------------------------------------------------------------------------------------------ 1: operator
_GOT = {}        # (h, w, lossy) -> the batch-3 result on the device, shared by tests 1 to 3


def _vjp(eng, h, w, lossy):
    if (h, w, lossy) not in _GOT:
        c = DA.adjoint_case(h, w)
        eng.set_domain_rect(h, w, *R.DOMAIN)
        _GOT[(h, w, lossy)] = eng.residual_vjp_medium(c["g"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV) if lossy else None, c["q"].to(DEV))
        torch.cuda.synchronize()
        eng.check_async_errors()
    return _GOT[(h, w, lossy)]


@pytest.mark.parametrize("lossy", [True, False])
@pytest.mark.parametrize("h,w", [(n, n) for n in LA.SQUARES] + list(LA.RECTANGLES))
def test_residual_vjp_medium_matches_float64_autograd(eng, h, w, lossy):
    c = DA.adjoint_case(h, w)
    got = _vjp(eng, h, w, lossy)
    assert not bool(torch.isnan(got).any())
    want, bar = (c["vjp_m"], c["bar_m"]) if lossy else (c["vjp_d"], c["bar_d"])
    err = SP.errors(got, want)
    ratio = err / bar
    print(f"DENSITY ADJOINT {h}x{w} k_sq_im {'given' if lossy else 'NULL'} (P, Q) rows {R.factor(w)} columns {R.factor(h)}: error / bar per cotangent "
          + ", ".join(f"{p} {float(e):.3e} / {float(b):.3e} = {float(r):.3f}" for p, e, b, r in zip(LA.PROBES, err, bar, ratio))
          + "; density share of the bar " + ", ".join(f"{float(s):.3e}" for s in c["share"]))
    assert bool((ratio <= 1.0).all()), ratio.tolist()
    # a sample's bits depend on neither its batch mates nor the lines per block its batch gives it
    eng.set_domain_rect(h, w, *R.DOMAIN)
    solo = eng.residual_vjp_medium(c["g"][1:2].to(DEV), c["k_sq"][1:2].to(DEV), c["k_sq_im"][1:2].to(DEV) if lossy else None, c["q"][1:2].to(DEV))
    assert torch.equal(solo[0], got[1])


# ------------------------------------------------------------------------------------------------------------------------- 2: inner product
@pytest.mark.parametrize("h,w", [(16, 16), (48, 48), (144, 144), (256, 256), (32, 80)])
def test_inner_product_identity_with_the_forward_density_operator(eng, h, w):
    c = DA.adjoint_case(h, w)
    for lossy in (True, False):
        vjp = _vjp(eng, h, w, lossy)
        eng.set_domain_rect(h, w, *R.DOMAIN)
        fwd = eng.residual_medium(c["u"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV) if lossy else None, c["q"].to(DEV),
                                  torch.zeros(1, 2, h, w, device=DEV))
        lhs = (fwd.cpu().double() * c["g"].double()).flatten(1).sum(1)
        rhs = (c["u"].double() * vjp.cpu().double()).flatten(1).sum(1)
        print(f"DENSITY ADJOINT {h}x{w} k_sq_im {'given' if lossy else 'NULL'} identity: "
              + ", ".join(f"{nm} <Au,g> {float(l):.6e} <u,A^H g> {float(r):.6e} |lhs-rhs| {abs(float(l - r)):.2e} bar {1e-5 * max(abs(float(l)), 1.0):.2e}"
                          for nm, l, r in zip(LA.PROBES, lhs, rhs)))
        for l, r in zip(lhs.tolist(), rhs.tolist()):
            assert abs(l - r) <= 1e-5 * max(abs(l), 1.0), (l, r)


# --------------------------------------------------------------------------------------------------------------------------- 3: zero gradient
@pytest.mark.parametrize("n", [16, 48, 144, 256])
def test_zero_density_gradient_agrees_with_the_constant_density_adjoints_and_two_calls_give_equal_bits(eng, n):
    c = DA.adjoint_case(n, n)
    eng.set_domain_rect(n, n, *R.DOMAIN)
    g, kq, ki, q = c["g"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV), c["q"].to(DEV)
    zero = torch.zeros_like(q)
    a, b = eng.residual_vjp_medium(g, kq, ki, zero), eng.residual_vjp_lossy(g, kq, ki)
    ratio = SP.peak(a.cpu().double() - b.cpu().double()) / (2 * c["bar"])
    print(f"DENSITY ADJOINT {n} q = 0 against hn_residual_vjp_lossy: error / (2 bar) " + ", ".join(f"{float(r):.3f}" for r in ratio))
    assert bool((ratio <= 1.0).all()), ratio.tolist()
    a, b = eng.residual_vjp_medium(g, kq, None, zero), eng.residual_vjp(g, kq)
    ratio = SP.peak(a.cpu().double() - b.cpu().double()) / (2 * LA.lossless_bar(c))
    print(f"DENSITY ADJOINT {n} q = 0, k_sq_im NULL against hn_residual_vjp: error / (2 bar) " + ", ".join(f"{float(r):.3f}" for r in ratio))
    assert bool((ratio <= 1.0).all()), ratio.tolist()
    for lossy in (True, False):
        assert torch.equal(eng.residual_vjp_medium(g, kq, ki if lossy else None, q), _vjp(eng, n, n, lossy))
        eng.set_domain_rect(n, n, *R.DOMAIN)
        assert torch.equal(eng.residual_vjp_medium(g, kq, ki if lossy else None, q), eng.residual_vjp_medium(g, kq, ki if lossy else None, q))


# ------------------------------------------------------------------------------------------------------------------------ 4: gradient kernel
@pytest.mark.parametrize("src_batch", [1, 3])
@pytest.mark.parametrize("n", [16, 48, 144])
def test_adjoint_grad_medium_kernel(eng, n, src_batch):
    """P = 1, 3, 9.  g_k_sq, g_k_sq_im and g_src are hn_adjoint_grad_lossy's bits (with g_k_sq_im NULL: hn_adjoint_grad's); g_rho_grad against the
    float64 ``density_common.first_derivatives`` with the tables' b_x / b_y, on seeded lam and u."""
    eng.set_domain_rect(n, n, *R.DOMAIN)
    gen = torch.Generator().manual_seed(11 * n + src_batch)
    lam, u = (torch.randn(3, 2, n, n, generator=gen).to(DEV) for _ in range(2))
    g_k, g_ki, g_q, g_s = eng.adjoint_grad_medium(lam, u, src_batch)
    old_k, old_ki, old_s = eng.adjoint_grad_lossy(lam, u, src_batch)
    assert torch.equal(g_k, old_k) and torch.equal(g_ki, old_ki) and torch.equal(g_s, old_s)          # hn_adjoint_grad_lossy's, bit for bit
    l_k, l_ki, l_q, l_s = eng.adjoint_grad_medium(lam, u, src_batch, lossy=False)
    ll_k, ll_s = eng.adjoint_grad(lam, u, src_batch)
    assert l_ki is None and torch.equal(l_k, ll_k) and torch.equal(l_s, ll_s) and torch.equal(l_q, g_q)
    again = eng.adjoint_grad_medium(lam, u, src_batch)
    assert all(torch.equal(a, b) for a, b in zip((g_k, g_ki, g_q, g_s), again))
    t = R.tables(n, n)
    ld, ud = lam.cpu().double(), u.cpu().double()
    dx, dy = DC.first_derivatives(ud, t)
    bx, by = O.complex_mul(t.bx, dx), O.complex_mul(t.by, dy)                                          # [B, n, n, 2]
    want = torch.stack([ld[:, 0] * bx[..., 0] + ld[:, 1] * bx[..., 1], ld[:, 0] * by[..., 0] + ld[:, 1] * by[..., 1]], 1)
    big = torch.maximum(bx.pow(2).sum(-1).sqrt().flatten(1).max(1).values, by.pow(2).sum(-1).sqrt().flatten(1).max(1).values)
    bar = SP.peak(ld) * (SP.BAR * DC.density_share(ud, torch.ones(3, 2, n, n, dtype=torch.float64), t) + 4e-7 * big)
    err = SP.errors(g_q, want)
    print(f"n={n} (P, Q) {R.factor(n)} src_batch={src_batch}: max |g_rho_grad - float64| per sample "
          + ", ".join(f"{float(e):.3e} / {float(b):.3e} = {float(e / b):.3f}" for e, b in zip(err, bar)) + f"; max |dJ/dq| {float(want.abs().max()):.3e}")
    assert tuple(g_q.shape) == (3, 2, n, n) and bool((err <= bar).all())
    none = eng.adjoint_grad_medium(lam, u, None)
    assert none[3] is None and torch.equal(none[0], g_k) and torch.equal(none[2], g_q)
    # a sample's bits do not depend on its batch mates
    assert torch.equal(eng.adjoint_grad_medium(lam[1:2].contiguous(), u[1:2].contiguous(), None)[2][0], g_q[1])
    # refusals leave the outputs alone
    keep = [x.clone() for x in (g_k, g_ki, g_q, g_s)]
    call = lambda l, uu, sb, b, gk, gki, gq, gs: eng.lib.hn_adjoint_grad_medium(eng.ctx, _p(l), _p(uu), sb, b, _p(gk), _p(gki), _p(gq), _p(gs),  # noqa: E731
                                                                               eng._stream())
    assert call(lam, u, 1, 3, g_k, g_ki, 0, 0) == ERR_ARG and "NULL" in _err(eng)
    assert call(lam, u, 1, 3, g_k, g_ki, g_q.data_ptr() + 4, 0) == ERR_ARG and "g_rho_grad is not 16-byte aligned" in _err(eng)
    assert call(lam, u, 1, 3, g_k, g_ki, g_k, 0) == ERR_ARG and "g_k_sq overlaps g_rho_grad" in _err(eng)
    assert call(lam, u, 1, 3, g_k, g_ki, lam, 0) == ERR_ARG and "lambda overlaps g_rho_grad" in _err(eng)
    assert call(lam, u, 2, 3, g_k, g_ki, g_q, 0) == ERR_ARG and "src batch" in _err(eng)
    eng.set_domain_rect(n, 2 * n, *R.DOMAIN)
    assert call(lam, u, 1, 3, g_k, g_ki, g_q, 0) == ERR_UNSUPPORTED and "rectangular domain" in _err(eng) and "hn_adjoint_grad_medium" in _err(eng)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((g_k, g_ki, g_q, g_s), keep))


# ------------------------------------------------------------------------------------------------------------------------------ 5: one cycle
def _cycle_problem(n, batch, rhs_batch, a0=0.1):
    s = _solver(n, (n // 2 - 2, n // 2))
    p = DA.ring_problem(n, a0, b=batch)
    src = s.source.detach().float().contiguous()
    if rhs_batch != 1:
        src = torch.cat([src * (1.0 + 0.5 * b) for b in range(rhs_batch)]).contiguous()
    return s, {k: p[k].to(DEV) for k in ("k_sq", "k_sq_im", "q", "rho")}, src


def _cyc(eng, adjoint, m, rhs, restart, tol, iters, alpha, x=None, rho="own"):
    b, n = m["k_sq"].shape[0], m["k_sq"].shape[-1]
    x = torch.zeros(b, 2, n, n, device=DEV) if x is None else x.clone()
    basis = torch.full((b, restart + 1, 2 * n * n), NAN, device=DEV)
    zbasis = torch.full((b, restart, 2 * n * n), NAN, device=DEV)
    hess = torch.full((b, restart + 1, restart, 2), NAN, device=DEV)
    if adjoint:
        rmse, k_used = eng.fgmres_adjoint_cycle_medium(x, m["k_sq"], m["k_sq_im"], m["q"], m["rho"] if isinstance(rho, str) else rho, rhs, restart, tol,
                                                       iters, alpha, basis=basis, zbasis=zbasis, hess=hess)
    else:
        rmse, k_used = eng.fgmres_cycle_medium(x, m["k_sq"], m["k_sq_im"], m["q"], rhs, restart, tol, iters, alpha, basis=basis, hess=hess, zbasis=zbasis)
    return {"x": x, "basis": basis, "zbasis": zbasis, "hess": hess, "rmse": rmse, "k_used": k_used}


_DENSE_UP_TO = 48      # the dense matrix of a sample: 85 MB at 48^2, 1.4 GB at 96^2
_DENSE = {}
_PIN = {}              # n -> the largest relative difference between the dense and the matrix-free float64 operator seen on the cycles' vectors


def _apply_free(adjoint, rows, m, b, n):
    f = torch.from_numpy(np.stack([rows.real, rows.imag], 1).reshape(rows.shape[0], 2, n, n))
    kq, ki, q = m["k_sq"][b:b + 1].double().cpu(), m["k_sq_im"][b:b + 1].double().cpu(), m["q"][b:b + 1].double().cpu()
    if adjoint:
        out = DA.adjoint_ref(f, kq, ki, q, n, n)
    else:
        with torch.no_grad():
            out = DC.residual(f, kq, ki, q, torch.zeros(1, 2, n, n, dtype=torch.float64), R.tables(n, n))
    return LA.np_complex(out)


def _apply64(adjoint, rows, m, b, n):
    """Rows of M v (or M^H v) for the complex rows v [k, P] in float64 on the host: by the dense ``DC.medium_matrix`` up to n = 48 (where the
    matrix-free operator is applied too and the two are compared), matrix-free above."""
    free = _apply_free(adjoint, rows, m, b, n)
    if n > _DENSE_UP_TO:
        return free
    if (n, b) not in _DENSE:
        _DENSE[(n, b)] = DC.medium_matrix(m["k_sq"][b, 0].cpu().numpy(), m["k_sq_im"][b, 0].cpu().numpy(), m["q"][b].cpu().numpy())
    M = _DENSE[(n, b)]
    dense = np.conj(np.conj(rows) @ M) if adjoint else rows @ M.T
    _PIN[n] = max(_PIN.get(n, 0.0), float(np.abs(dense - free).max() / np.abs(dense).max()))
    return dense


def _iterates(Zc, Hc, beta, restart):
    out = []
    for j in range(1, restart + 1):
        e1 = np.zeros(j + 1, np.complex128); e1[0] = beta
        y = np.linalg.lstsq(Hc[: j + 1, :j], e1, rcond=None)[0]
        out.append((y[:, None] * Zc[:j]).sum(0))
    return np.stack(out)


def _invariants(run, adjoint, n, m, rhs, restart):
    """(max |V^H V - I|, max |Op Z - V_{m+1} H| / max |H|, max_j |rmse[j] - true RMSE of the j-step iterate rebuilt in float64 from Z and H| / rmse[0])
    over the batch; the iterates start from x = 0."""
    orth = arn = dev = 0.0
    for b in range(m["k_sq"].shape[0]):
        Vc, Zc = LA.np_complex(run["basis"][b]), LA.np_complex(run["zbasis"][b])
        Hc = run["hess"][b].double().cpu().numpy()
        Hc = Hc[..., 0] + 1j * Hc[..., 1]
        orth = max(orth, float(np.abs(Vc.conj() @ Vc.T - np.eye(restart + 1)).max()))
        arn = max(arn, float(np.abs(_apply64(adjoint, Zc, m, b, n) - Hc.T @ Vc).max() / np.abs(Hc).max()))
        g = LA.np_complex(rhs[b if rhs.shape[0] > 1 else 0])
        beta = float(np.linalg.norm(g))
        res = g[None] - _apply64(adjoint, _iterates(Zc, Hc, beta, restart), m, b, n)
        true = np.concatenate([[beta], np.linalg.norm(res, axis=1)]) / np.sqrt(2.0 * n * n)
        dev = max(dev, float(np.abs(run["rmse"][:, b].double().cpu().numpy() - true).max() / true[0]))
    return orth, arn, dev


@pytest.mark.parametrize("n,rhs_batch", [(48, 1), (96, 2)])
def test_arnoldi_invariants_of_one_plain_density_adjoint_cycle(n, rhs_batch):
    """precond_iters = 0, rho NULL: plain restarted GMRES on A_rho^H.  The invariants of test_arnoldi_invariants_of_one_plain_lossy_adjoint_cycle at
    4 x what hn_fgmres_cycle_medium shows on the forward system; zbasis == basis bit for bit; rho is not read (a plane of NaN changes nothing)."""
    restart, batch = 5, 2
    s, m, rhs = _cycle_problem(n, batch, rhs_batch)
    eng = s.engine()
    adj = _cyc(eng, True, m, rhs, restart, 0.0, 0, 1.0, rho=None)
    fwd = _cyc(eng, False, m, rhs, restart, 0.0, 0, 1.0)
    assert adj["k_used"].tolist() == [restart] * batch
    for key in ("basis", "zbasis", "hess", "rmse"):
        assert bool(torch.isfinite(adj[key]).all()), key
    assert torch.equal(adj["zbasis"], adj["basis"][:, :restart])
    got = _invariants(adj, True, n, m, rhs, restart)
    ref = _invariants(fwd, False, n, m, rhs, restart)
    names = ("orthogonality", "arnoldi relation", "rmse estimate")
    for name, a, r in zip(names, got, ref):
        print(f"n={n} rhs_batch={rhs_batch} {name}: density adjoint {a:.3e}  density forward {r:.3e}  bar {4 * r:.3e}")
    for name, a, r in zip(names, got, ref):
        assert a <= 4 * r, (name, a, r)
    if n <= _DENSE_UP_TO:
        print(f"n={n}: dense M / M^H against the matrix-free float64 operator on the cycles' vectors: {_PIN[n]:.3e} of the largest entry, bar 1e-12")
        assert _PIN[n] <= 1e-12
    again = _cyc(eng, True, m, rhs, restart, 0.0, 0, 1.0, rho=torch.full_like(m["rho"], NAN))
    for key in adj:
        assert torch.equal(adj[key], again[key]), key


def test_only_ratios_of_rho_enter_the_preconditioner():
    """n = 48, two samples with the same medium and right-hand side, the second with rho * 1000, one preconditioned cycle (2 inner steps of 2 network
    iterations): the z vectors agree to fp32 rounding.  Bar 1e-5 * max|z|: the two samples' normalised planes rho / rho[0, 0] differ by at most three
    roundings (1.8e-7, relative, pointwise) going in and again coming out, 3.6e-7 together; the two network iterations between them are allowed to
    amplify a perturbation of their right-hand side by 25 -- they are a contraction towards A^-1 src on the magnitudes they were trained on, and
    z / max|z| is of order one -- which gives 1e-5.  A dependence on the scale itself would show at order one (without the normalisation the network
    would see a right-hand side 1000 x what it was trained on), a partial one (a factor forgotten on one side) at 1e-3 or more."""
    n, restart = 48, 2
    s, m, rhs = _cycle_problem(n, 1, 1)
    eng = s.engine()
    two = {k: torch.cat([v, v]).contiguous() for k, v in m.items()}
    two["rho"] = torch.cat([m["rho"], m["rho"] * 1000.0]).contiguous()
    run = _cyc(eng, True, two, rhs, restart, 0.0, 2, _alpha_scale(rhs))
    z = run["zbasis"].double()
    assert bool(torch.isfinite(z).all()) and not torch.equal(run["zbasis"], run["basis"][:, :restart])
    diff, scale = float((z[0] - z[1]).abs().max()), float(z[0].abs().max())
    print(f"n={n}: max |z(rho) - z(1000 rho)| = {diff:.3e}, max|z| = {scale:.3e}, ratio {diff / scale:.3e}, bar 1e-5")
    assert diff <= 1e-5 * scale


# -------------------------------------------------------------------------------------------------------------------------- 6: adjoint solve
@pytest.mark.parametrize("precondition", [None, "learned"])
@pytest.mark.parametrize("n,loc", [(32, (12, 16)), (48, (14, 24))])
def test_adjoint_solve_vs_float64_direct_solve(n, loc, precondition):
    a0 = 0.1
    s = _solver(n, loc)
    p = DA.ring_problem(n, a0)
    g = LA.scaled_field((2, 2, n, n), 100 + n, float(torch.linalg.vector_norm(s.source.detach().double()))).to(DEV)
    out = s.adjoint_solve(g, p["sos"].to(DEV), precondition=precondition, restart=40, max_outer=60, tol=2e-6, precond_iterations=10,
                          absorption=p["alpha"].to(DEV), density=p["rho"].to(DEV))
    print(f"n={n} a0={a0} {precondition}: cycles {out['cycles']} iterations per sample {out['iterations_per_sample'].tolist()} converged "
          f"{out['converged']} true rmse {out['residual_norm'].tolist()} unet evaluations {out['unet_evaluations']}")
    assert out["converged"]
    got = LA.np_complex(out["wavefield"])
    for b in range(2):
        M = DC.medium_matrix(p["k_sq"][b, 0].numpy(), p["k_sq_im"][b, 0].numpy(), p["q"][b].numpy())
        want = np.linalg.solve(M.conj().T, LA.np_complex(g[b]))
        err = max(np.abs(got[b].real - want.real).max(), np.abs(got[b].imag - want.imag).max())
        scale = max(np.abs(want.real).max(), np.abs(want.imag).max())
        print(f"n={n} a0={a0} {precondition} sample {b}: max|lam - lam64| = {err:.3e}, bar {2e-4 * scale:.3e}")
        assert err <= 2e-4 * scale, (b, err, scale)


# ------------------------------------------------------------------------------------------------------------------ 7: gradients end to end
def _maxabs(c):
    return max(np.abs(c.real).max(), np.abs(c.imag).max())


@pytest.mark.parametrize("n,loc", [(32, (12, 16)), (48, (14, 24))])
def test_implicit_gradients_vs_float64(n, loc):
    """solve_implicit(absorption = a tensor, density = a tensor, tol 2e-6, restart 40, 60 cycles) + backward on the three-map ring media with
    a0 = 0.1, the receiver-row loss; sos.grad, alpha.grad, rho.grad and source.grad against the dense float64 adjoint-state values and a central
    difference (h 1e-6) of the float64 direct-solve loss: |<e, delta>| <= max|e| sum|delta| with the gradient's bar for max|e|.

    Bars: base = 4e-4 max|lam| max|u| (2e-4 of either solve) times a chain factor.  For sos and alpha the factors of test_lossy_adjoint_gpu.  For rho:
    dJ/dq = Re(conj(lam) b D u) with |b D u| <= max|b| ||D||_inf max|u| and |b D du| <= max|b| ||D||_inf max|du| gives base * chain_q,
    chain_q = max|b| ||D||_inf; dJ/drho = -(G_x dJ/dq_x + G_y dJ/dq_y) / rho then gives chain_rho = chain_q (||G_x||_inf + ||G_y||_inf) / min rho,
    || ||_inf the largest absolute row sum of the axis matrix (density_adjoint_common.gradient_reference).

    chain_rho is 84 ... 106, so that bar alone would let a 10 % error of the chain from dJ/dq to rho through.  The chain is therefore pinned on its
    own: rho.grad against float64 autograd through the restated q(rho) applied to the DEVICE's dJ/dq (the bits hn_adjoint_grad_medium returns for the
    same lam and u -- the adjoint solve is deterministic), bar 4e-7 * max|rho.grad|: the chain runs in float64 and is rounded to fp32 once, and the
    reference takes the fp32 dJ/dq exactly; 4e-7 leaves room for a second rounding."""
    a0 = 0.1
    s = _solver(n, loc)
    eng = s.engine()
    src = LA.np_complex(s.source.detach()[0])
    ref = DA.gradient_reference(n, a0, src)
    p = DA.ring_problem(n, a0)
    rx = ref["rx"]
    d = torch.from_numpy(np.stack([np.stack([x.real, x.imag]) for x in ref["d"]]).astype(np.float32)).to(DEV)      # [2, 2, n]
    sos = p["sos"].to(DEV).requires_grad_(True)
    alpha = p["alpha"].to(DEV).requires_grad_(True)
    rho = p["rho"].to(DEV).requires_grad_(True)
    s.source.requires_grad_(True)
    try:
        out = s.solve_implicit(sos, absorption=alpha, density=rho, tol=2e-6, restart=40, max_cycles=60)
        u = out["wavefield"]
        assert u.requires_grad and out["converged"] and out["adjoint"] == {}
        loss = 0.5 * ((u[:, :, rx, :] - d) ** 2).sum()
        loss.backward()
        with pytest.raises(RuntimeError, match="create_graph"):
            out2 = s.solve_implicit(sos, absorption=alpha, density=rho, tol=1e-3, restart=10, max_cycles=5)
            torch.autograd.grad(out2["wavefield"].sum(), rho, create_graph=True)
        g_sos, g_alpha, g_rho = (t.grad.detach().double().cpu().numpy() for t in (sos, alpha, rho))
        g_src = s.source.grad.detach().clone()
    finally:
        s.source.requires_grad_(False)
        s.source.grad = None
    info = out["adjoint"]
    print(f"n={n}: forward cycles {len(out['cycle_tables'])}, adjoint {info['cycles']} cycles, converged {info['converged']}, true rmse "
          f"{info['rmse'].tolist()}, unet evaluations {info['unet_evaluations']}")
    assert info["converged"] and float(info["rmse"].max()) < 2e-6
    # dJ/dk_sq, dJ/dk_sq_im and dJ/dq by the same two calls backward makes: the adjoint solve of the loss's cotangent, then hn_adjoint_grad_medium
    cot = torch.zeros_like(u.detach()); cot[:, :, rx, :] = u.detach()[:, :, rx, :] - d
    lam = s.adjoint_solve(cot.contiguous(), sos.detach(), restart=40, max_outer=60, tol=2e-6, precondition="learned", absorption=alpha.detach(),
                          density=rho.detach())["wavefield"]
    dev_out = eng.adjoint_grad_medium(lam, u.detach().contiguous(), None)
    g_k, g_ki, g_q, _ = (t if t is None else t.double().cpu().numpy() for t in dev_out)
    chain = DA.rho_chain_ref(dev_out[2].cpu(), p["rho"]).numpy()
    e_chain, top = float(np.abs(g_rho - chain).max()), float(np.abs(chain).max())
    print(f"n={n}: rho.grad against the float64 chain of the device's own dJ/dq: {e_chain:.3e}, bar {4e-7 * top:.3e} (max|rho.grad| {top:.3e})")
    assert e_chain <= 4e-7 * top
    src_bar = 0.0
    for b in range(2):
        ml, mu = _maxabs(ref["lam"][b]), _maxabs(ref["u"][b])
        base = 4e-4 * ml * mu
        errs = {"g_k_sq": (np.abs(g_k[b, 0] - ref["g_k_sq"][b]).max(), base), "g_k_sq_im": (np.abs(g_ki[b, 0] - ref["g_k_sq_im"][b]).max(), base),
                "g_rho_grad": (np.abs(g_q[b] - ref["g_q"][b]).max(), base * ref["chain_q"][b]),
                "sos.grad": (np.abs(g_sos[b, 0] - ref["g_sos"][b]).max(), base * ref["chain_sos"][b]),
                "alpha.grad": (np.abs(g_alpha[b, 0] - ref["g_alpha"][b]).max(), base * ref["chain_alpha"][b]),
                "rho.grad": (np.abs(g_rho[b, 0] - ref["g_rho"][b]).max(), base * ref["chain_rho"][b])}
        print(f"n={n} sample {b}: max|lam| {ml:.3e} max|u| {mu:.3e} chain_q {ref['chain_q'][b]:.3f} chain_rho {ref['chain_rho'][b]:.3f} "
              f"max|dJ/drho| {np.abs(ref['g_rho'][b]).max():.3e}; " + "; ".join(f"{k} error {e:.3e}, bar {bar:.3e}" for k, (e, bar) in errs.items()))
        for k, (e, bar) in errs.items():
            assert e <= bar, (k, e, bar)
        src_bar += 2e-4 * ml
        sb, ab, rb = p["sos"][b, 0].double().numpy(), p["alpha"][b, 0].double().numpy(), p["rho"][b:b + 1].double()
        M, q0, h = ref["M"][b], ref["q"][b], 1e-6
        for name, grad, chain, moved in (("sos", g_sos, ref["chain_sos"][b], 0), ("alpha", g_alpha, ref["chain_alpha"][b], 1)):
            delta = np.random.default_rng(300 + n + b + 10 * moved).standard_normal((n, n))
            plus = (sb + h * delta, ab) if moved == 0 else (sb, ab + h * delta)
            minus = (sb - h * delta, ab) if moved == 0 else (sb, ab - h * delta)
            fd = (LA.loss64(M, sb, ab, *plus, src, rx, ref["d"][b]) - LA.loss64(M, sb, ab, *minus, src, rx, ref["d"][b])) / (2 * h)
            an = float((grad[b, 0] * delta).sum())
            bar = base * chain * float(np.abs(delta).sum())
            print(f"n={n} sample {b}: <{name}.grad, delta> {an:.8e}  central difference {fd:.8e}  difference {abs(an - fd):.3e}, bar {bar:.3e}")
            assert abs(an - fd) <= bar
        # rho: perturb rho, recompute q in float64; the operator is linear in q, so only q's change enters
        delta = np.random.default_rng(330 + n + b).standard_normal((n, n))
        q_of = lambda r: DA.log_gradient_torch(r)[0].numpy()  # noqa: E731
        qc = q_of(rb)
        fd = (DA.loss64(M, q0, q0 + (q_of(rb + h * torch.from_numpy(delta)) - qc), src, rx, ref["d"][b])
              - DA.loss64(M, q0, q0 + (q_of(rb - h * torch.from_numpy(delta)) - qc), src, rx, ref["d"][b])) / (2 * h)
        an = float((g_rho[b, 0] * delta).sum())
        bar = base * ref["chain_rho"][b] * float(np.abs(delta).sum())
        print(f"n={n} sample {b}: <rho.grad, delta> {an:.8e}  central difference {fd:.8e}  difference {abs(an - fd):.3e}, bar {bar:.3e}")
        assert abs(an - fd) <= bar
    got_src = LA.np_complex(g_src[0])
    e = max(np.abs(got_src.real - ref["g_src"].reshape(-1).real).max(), np.abs(got_src.imag - ref["g_src"].reshape(-1).imag).max())
    print(f"n={n}: source.grad error {e:.3e}, bar {src_bar:.3e}")
    assert tuple(g_src.shape) == (1, 2, n, n) and e <= src_bar


def test_density_without_absorption_and_a_density_that_does_not_require_grad():
    """n = 32, no absorption (the k_sq_im NULL route end to end): sos.grad and rho.grad against the dense float64 values of the medium with alpha = 0,
    at the bars of test_implicit_gradients_vs_float64; one rho for the batch receives the sum over it; a density that does not require grad gets
    none and sos.grad is the same bits."""
    n, loc = 32, (12, 16)
    s = _solver(n, loc)
    src = LA.np_complex(s.source.detach()[0])
    ref = DA.gradient_reference(n, 0.0, src)
    p = DA.ring_problem(n, 0.0)
    rx = ref["rx"]
    d = torch.from_numpy(np.stack([np.stack([x.real, x.imag]) for x in ref["d"]]).astype(np.float32)).to(DEV)
    grads = {}
    for needs in (True, False):
        sos = p["sos"].to(DEV).requires_grad_(True)
        rho = p["rho"].to(DEV).requires_grad_(needs)
        out = s.solve_implicit(sos, density=rho, tol=2e-6, restart=40, max_cycles=60)
        (0.5 * ((out["wavefield"][:, :, rx, :] - d) ** 2).sum()).backward()
        assert out["converged"] and out["adjoint"]["converged"] and s.source.grad is None
        grads[needs] = (sos.grad.detach().clone(), None if rho.grad is None else rho.grad.detach().clone())
    assert grads[False][1] is None and torch.equal(grads[False][0], grads[True][0])
    g_sos, g_rho = (t.double().cpu().numpy() for t in grads[True])
    for b in range(2):
        base = 4e-4 * _maxabs(ref["lam"][b]) * _maxabs(ref["u"][b])
        for name, e, bar in (("sos.grad", np.abs(g_sos[b, 0] - ref["g_sos"][b]).max(), base * ref["chain_sos"][b]),
                             ("rho.grad", np.abs(g_rho[b, 0] - ref["g_rho"][b]).max(), base * ref["chain_rho"][b])):
            print(f"n={n} no absorption, sample {b}: {name} error {e:.3e}, bar {bar:.3e}")
            assert e <= bar
    # one density map for the whole batch: the sum over the samples it was broadcast to (both samples then share sample 0's density)
    one = p["rho"][:1].to(DEV).requires_grad_(True)
    sos = p["sos"][:1].expand(2, -1, -1, -1).contiguous().to(DEV)
    out = s.solve_implicit(sos, density=one, tol=2e-6, restart=40, max_cycles=60)
    (0.5 * ((out["wavefield"][:, :, rx, :] - d[:1]) ** 2).sum()).backward()
    per = p["rho"][:1].expand(2, -1, -1, -1).contiguous().to(DEV).requires_grad_(True)
    out = s.solve_implicit(sos, density=per, tol=2e-6, restart=40, max_cycles=60)
    (0.5 * ((out["wavefield"][:, :, rx, :] - d[:1]) ** 2).sum()).backward()
    assert tuple(one.grad.shape) == (1, 1, n, n)
    e, scale = float((one.grad[0] - (per.grad[0] + per.grad[1])).abs().max()), float(one.grad.abs().max())
    print(f"n={n}: one rho for two samples against the sum of the per-sample gradients: {e:.3e} of {scale:.3e}, bar {4e-7 * scale:.3e} (one fp32 sum)")
    assert e <= 4e-7 * scale


# ---------------------------------------------------------------------------------------------------------------------- 8: refusals and order
def _raw_cycle(eng, x, k_sq, k_im, q, rho, rhs, rhs_batch, batch, restart, tol, m, alpha, basis, zbasis, hess, rmse, k_used):
    return eng.lib.hn_fgmres_adjoint_cycle_medium(eng.ctx, _p(x), _p(k_sq), _p(k_im), _p(q), _p(rho), _p(rhs), rhs_batch, batch, restart, tol, m, alpha,
                                                  _p(basis), _p(zbasis), _p(hess), _p(rmse), _p(k_used), eng._stream())


def _buffers(h, w, batch, restart):
    f = lambda *shape: torch.full(shape, NAN, device=DEV)  # noqa: E731
    return (torch.zeros(batch, 2, h, w, device=DEV), f(batch, restart + 1, 2 * h * w), f(batch, restart, 2 * h * w),
            f(batch, restart + 1, restart, 2), f(restart + 1, batch), torch.full((batch,), -7, device=DEV, dtype=torch.int32))


def _left_alone(bufs):
    torch.cuda.synchronize()
    assert float(bufs[0].abs().max()) == 0.0
    for t in bufs[1:-1]:
        assert bool(torch.isnan(t).all())
    assert bool((bufs[-1] == -7).all())


def test_argument_refusals(eng):
    h, w = 32, 80
    eng.set_domain_rect(h, w, *R.DOMAIN)
    c = DA.adjoint_case(h, w)
    g, kq, ki, q = c["g"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV), c["q"].to(DEV)
    out = torch.full_like(g, NAN)
    vjp = lambda g_, kq_, ki_, q_, out_, b: eng.lib.hn_residual_vjp_medium(eng.ctx, _p(g_), _p(kq_), _p(ki_), _p(q_), _p(out_), b, eng._stream())  # noqa: E731
    assert vjp(g, kq, ki, 0, out, 3) == ERR_ARG and "rho_grad is NULL" in _err(eng) and "hn_residual_vjp_lossy" in _err(eng) and "hn_residual_vjp " in _err(eng)
    assert vjp(g, 0, ki, q, out, 3) == ERR_ARG and "NULL" in _err(eng)
    assert vjp(g, kq, ki, q, out, 0) == ERR_ARG and "batch" in _err(eng)
    assert vjp(g, kq, ki, q, g, 3) == ERR_ARG and "alias" in _err(eng)
    assert vjp(g, kq, 0, q, g, 3) == ERR_ARG and "alias" in _err(eng)
    assert vjp(g, kq, out.data_ptr() + 64, q, out, 1) == ERR_ARG and "k_sq_im overlaps out" in _err(eng)
    assert vjp(g, kq, ki, out.data_ptr() + 64, out, 1) == ERR_ARG and "rho_grad overlaps out" in _err(eng)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the cycle: NULL rho_grad names the constant-density siblings; a rectangular domain is unsupported
    bufs = _buffers(h, w, 3, 4)
    x, basis, zbasis, hess, rmse, k_used = bufs
    rhs, rho = torch.zeros(1, 2, h, w, device=DEV), torch.ones(3, 1, h, w, device=DEV)
    assert _raw_cycle(eng, x, kq, ki, 0, rho, rhs, 1, 3, 4, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used) == ERR_ARG
    assert "hn_fgmres_adjoint_cycle_lossy" in _err(eng) and "rho_grad is NULL" in _err(eng)
    assert _raw_cycle(eng, x, kq, ki, q, rho, rhs, 1, 3, 4, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used) == ERR_UNSUPPORTED
    assert "rectangular domain" in _err(eng) and "hn_fgmres_adjoint_cycle_medium" in _err(eng)
    _left_alone(bufs)
    # on a square domain: rho by k_sq's rules, and required by the preconditioner alone
    n = 32
    eng.set_domain_rect(n, n, *R.DOMAIN)
    bufs = _buffers(n, n, 2, 3)
    x, basis, zbasis, hess, rmse, k_used = bufs
    kq, ki, rhs = torch.ones(2, 1, n, n, device=DEV), torch.zeros(2, 1, n, n, device=DEV), torch.zeros(1, 2, n, n, device=DEV)
    q, rho = torch.zeros(2, 2, n, n, device=DEV), torch.ones(2, 1, n, n, device=DEV)
    call = lambda **kw: _raw_cycle(eng, **{**dict(x=x, k_sq=kq, k_im=ki, q=q, rho=rho, rhs=rhs, rhs_batch=1, batch=2, restart=3, tol=0.0, m=0, alpha=1.0,  # noqa: E731
                                                  basis=basis, zbasis=zbasis, hess=hess, rmse=rmse, k_used=k_used), **kw})
    assert call(rho=0, m=1) == ERR_ARG and "rho is NULL" in _err(eng) and "hn_fgmres_adjoint_cycle_medium" in _err(eng)
    assert call(rho=0, m=3) == ERR_ARG and "rho is NULL" in _err(eng)
    assert call(rho=rho.data_ptr() + 4) == ERR_ARG and "rho is not 16-byte aligned" in _err(eng)
    assert call(rho=kq) == ERR_ARG and "rho overlaps k_sq" in _err(eng)
    assert call(rho=basis) == ERR_ARG and "rho overlaps basis" in _err(eng)
    assert call(q=q.data_ptr() + 4) == ERR_ARG and "rho_grad is not 16-byte aligned" in _err(eng)
    assert call(q=rho) == ERR_ARG and "rho_grad overlaps rho" in _err(eng)
    assert call(k_im=ki.data_ptr() + 4) == ERR_ARG and "k_sq_im is not 16-byte aligned" in _err(eng)
    assert call(restart=0) == ERR_ARG and "restart" in _err(eng)
    assert call(m=-1) == ERR_ARG and "precond_iters" in _err(eng)
    assert call(zbasis=0) == ERR_ARG and "NULL" in _err(eng)
    _left_alone(bufs)
    with pytest.raises(RuntimeError, match="grad"):
        eng.fgmres_adjoint_cycle_medium(x, kq, ki, q, rho.clone().requires_grad_(True), rhs, 3, 0.0, 0, 1.0)
    with pytest.raises(RuntimeError, match="grad"):
        eng.fgmres_adjoint_cycle_medium(x, kq, ki, q.clone().requires_grad_(True), rho, rhs, 3, 0.0, 0, 1.0)


def test_first_gradient_call_under_stream_capture_is_refused_and_the_capture_ends_clean():
    n = 64
    e = _engine()
    e.set_domain_rect(n, n, *R.DOMAIN)          # a power of two: the lossless routes build no line tables
    gen = torch.Generator().manual_seed(4)
    lam, u = (torch.randn(2, 2, n, n, generator=gen).to(DEV) for _ in range(2))
    g_k, g_ki = torch.full((2, 1, n, n), NAN, device=DEV), torch.full((2, 1, n, n), NAN, device=DEV)
    g_q = torch.full((2, 2, n, n), NAN, device=DEV)
    probe = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probe.add_(1.0)
        rc = e.lib.hn_adjoint_grad_medium(e.ctx, _p(lam), _p(u), 1, 2, _p(g_k), _p(g_ki), _p(g_q), _p(0), e._stream())
        msg = _err(e)
    assert rc == ERR_STATE and "captur" in msg and "hn_adjoint_grad_medium" in msg
    graph.replay()                                # the capture is still valid, and holds nothing of the library's
    torch.cuda.synchronize()
    assert probe.tolist() == [1.0] * 4 and all(bool(torch.isnan(t).all()) for t in (g_k, g_ki, g_q))
    got = e.adjoint_grad_medium(lam, u, None)     # eager: builds the tables
    other = _engine()                             # a context that was never refused
    other.set_domain_rect(n, n, *R.DOMAIN)
    want = other.adjoint_grad_medium(lam, u, None)
    assert all(bool(torch.isfinite(a).all()) and torch.equal(a, b) for a, b in zip(got[:3], want[:3]))
    # a later call is capturable, and the replay gives the eager bits
    out = [torch.full_like(t, NAN) for t in (g_k, g_ki, g_q)]
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        rc = e.lib.hn_adjoint_grad_medium(e.ctx, _p(lam), _p(u), 1, 2, _p(out[0]), _p(out[1]), _p(out[2]), _p(0), e._stream())
    assert rc == OK
    graph2.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, got[:3]))
    for x in (e, other):
        torch.cuda.synchronize()
        x.check_async_errors()
        x.close()


# ------------------------------------------------------------------------------------------------------------------- 9: nothing else moved
def _family(e, n, case):
    """hn_residual_vjp, hn_residual_vjp_lossy, hn_residual_medium and one hn_fgmres_adjoint_cycle[_lossy] each, on seeded inputs."""
    u, kq, ki, q, src = case
    out = {"vjp": e.residual_vjp(u, kq), "vjp_lossy": e.residual_vjp_lossy(u, kq, ki), "medium": e.residual_medium(u, kq, ki, q, src)}
    for name, planes in (("", (kq,)), ("_lossy", (kq, ki))):
        x = torch.zeros_like(u)
        basis, zbasis = torch.zeros(u.shape[0], 4, 2 * n * n, device=DEV), torch.zeros(u.shape[0], 3, 2 * n * n, device=DEV)
        hess = torch.zeros(u.shape[0], 4, 3, 2, device=DEV)
        rmse, k_used = getattr(e, "fgmres_adjoint_cycle" + name)(x, *planes, src, 3, 0.0, 2, _alpha_scale(src), basis=basis, zbasis=zbasis, hess=hess)
        out.update({"x" + name: x, "basis" + name: basis, "zbasis" + name: zbasis, "hess" + name: hess, "rmse" + name: rmse, "k_used" + name: k_used})
    torch.cuda.synchronize()
    e.check_async_errors()
    return out


@pytest.mark.parametrize("n", [64, 144])
def test_the_constant_density_adjoints_and_the_forward_density_operator_are_untouched(blob, n):
    """A context that has run the three new calls against a fresh one, bit for bit: 64 (radix-4; the line tables built by the new calls) and 144, the
    mixed route that shares its axis tables and the <., true> instances with the new adjoint."""
    gen = torch.Generator().manual_seed(n)
    u = torch.randn(2, 2, n, n, generator=gen).to(DEV)
    kq, ki = R.seeded_k_sq(n, n, 2, 10 + n).to(DEV), LC.seeded_k_sq_im(n, n, 2, 20 + n).to(DEV)
    q = DC.seeded_q(n, n, 2).to(DEV)
    rho = (1.0 + torch.rand(2, 1, n, n, generator=gen)).to(DEV)
    src = R.point_source_map(n, n, [n // 4, n // 2], 10.0).to(DEV).contiguous()
    case = (u, kq, ki, q, src)
    fresh, used = _engine(blob), _engine(blob)
    for e in (fresh, used):
        e.set_domain_rect(n, n, *R.DOMAIN)
    g = used.residual_vjp_medium(u, kq, ki, q)
    run = _cyc(used, True, {"k_sq": kq, "k_sq_im": ki, "q": q, "rho": rho}, src, 3, 0.0, 2, _alpha_scale(src))
    used.adjoint_grad_medium(run["x"], g, 1)
    torch.cuda.synchronize()
    used.check_async_errors()
    assert bool(torch.isfinite(run["x"]).all())
    a, b = _family(fresh, n, case), _family(used, n, case)
    for key in a:
        assert bool(torch.isfinite(a[key].float()).all()), key
        assert torch.equal(a[key], b[key]), key
    fresh.close()
    used.close()
