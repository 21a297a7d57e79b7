"""The lossy adjoint operator and the adjoint-state gradients of an absorbing medium on the GPU: hn_residual_vjp_lossy, hn_fgmres_adjoint_cycle_lossy,
hn_adjoint_grad_lossy, ``gmres_adjoint(absorption=)`` and ``IterativeSolver.solve_implicit(absorption=)`` against the float64 references composed
in tests/lossy_adjoint_common.py.  Needs a real MI355X.  Every figure is printed beside its bar before it is asserted (pytest -s).

Bars:
    operator        SP.BAR * (scale * max|g| + max(|k~^2| |g|)): ``lossy_common.forward_case``'s without a source; with k_sq_im = 0 twice the lossless
                    bar against hn_residual_vjp (two fp32 routes, each within one bar of float64)
    inner product   |<A u, g> - <u, A^H g>| <= 1e-5 * max(|<A u, g>|, 1), summed in float64 (test_spectral_gpu's)
    one cycle       4 x what hn_fgmres_cycle_lossy shows for the same invariant on the forward system with the same planes, rhs and settings (the rule of
                    test_adjoint_gpu).  At n = 48 the operator of either check is the dense float64 matrix M (M^H for the adjoint cycle); at n = 96,
                    where M has 1.4 GB per sample, the float64 operator of tests/lossy_common.py applied matrix-free, which the n = 48 cases pin to
                    the dense one on the cycle's own vectors to 1e-12 of the largest entry
    adjoint solve   max|lam - lam64| <= 2e-4 * max|lam64| against solve(M^H, g) in float64
    pointwise       4e-7 * max|lam| * max|u| (a two-term fp32 product sum: three roundings of 6e-8 on terms bounded by max|lam| max|u|)
    gradients       4e-4 * max|lam| * max|u| on dJ/dk_sq and dJ/dk_sq_im (2e-4 of either solve, as test_adjoint_gpu), times the chain factors
                    max((2 k + 2 alpha) omega / c^2) for sos.grad and max(2 alpha + 2 k) for alpha.grad; 2e-4 max|lam| per sample on source.grad --
                    the one source map the two samples share receives lam_0 + lam_1, so its bar is the SUM of the two samples' bars
"""
import ctypes

import numpy as np
import pytest
import torch

import lossy_adjoint_common as LA
import lossy_common as LC
import rect_common as R
import spectral_probes as SP

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
_GOT = {}        # (h, w) -> the batch-3 result on the device, shared by tests 1 to 3


def _vjp(eng, h, w):
    if (h, w) not in _GOT:
        c = LA.adjoint_case(h, w)
        eng.set_domain_rect(h, w, *R.DOMAIN)
        _GOT[(h, w)] = eng.residual_vjp_lossy(c["g"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV))
        torch.cuda.synchronize()
        eng.check_async_errors()
    return _GOT[(h, w)]


@pytest.mark.parametrize("h,w", [(n, n) for n in LA.SQUARES] + list(LA.RECTANGLES))
def test_residual_vjp_lossy_matches_float64_autograd(eng, h, w):
    c = LA.adjoint_case(h, w)
    assert bool((c["k_sq_im"][1] <= 0).all()) and bool((c["k_sq_im"][0] >= 0).all())      # one sample with the amplifying sign
    got = _vjp(eng, h, w)
    assert not bool(torch.isnan(got).any())
    ratio = SP.errors(got, c["vjp"]) / c["bar"]
    print(f"LOSSY ADJOINT {h}x{w} (P, Q) rows {R.factor(w)} columns {R.factor(h)}: error / bar per cotangent "
          + ", ".join(f"{p} {float(e):.3e} / {float(b):.3e} = {float(r):.3f}" for p, e, b, r in zip(LA.PROBES, SP.errors(got, c["vjp"]), c["bar"], ratio)))
    assert bool((ratio <= 1.0).all()), ratio.tolist()
    # a sample's bits depend on neither its batch mates nor the lines per block its batch gives it
    eng.set_domain_rect(h, w, *R.DOMAIN)
    solo = eng.residual_vjp_lossy(c["g"][1:2].to(DEV), c["k_sq"][1:2].to(DEV), c["k_sq_im"][1:2].to(DEV))
    assert torch.equal(solo[0], got[1])


def test_the_large_lds_launch_gives_the_bits_of_the_small_one(eng):
    """n = 208 = 13 * 16 at batch 40: 16 lines per block in three buffers, 79.9 KB of dynamic LDS -- above the 64 KB a kernel may ask for without the
    attribute.  The samples repeat the three cotangents and must equal the batch-3 run (one line per block) bit for bit."""
    n, batch = 208, 40
    c = LA.adjoint_case(n, n)
    want = _vjp(eng, n, n)
    eng.set_domain_rect(n, n, *R.DOMAIN)
    idx = torch.arange(batch) % len(LA.PROBES)
    got = eng.residual_vjp_lossy(c["g"][idx].contiguous().to(DEV), c["k_sq"][idx].contiguous().to(DEV), c["k_sq_im"][idx].contiguous().to(DEV))
    torch.cuda.synchronize()
    eng.check_async_errors()
    assert not bool(torch.isnan(got).any())
    for s in range(batch):
        assert torch.equal(got[s], want[int(idx[s])]), s


# ------------------------------------------------------------------------------------------------------------------------- 2: inner product
@pytest.mark.parametrize("h,w", [(16, 16), (48, 48), (144, 144), (256, 256), (32, 80)])
def test_inner_product_identity_with_the_forward_lossy_operator(eng, h, w):
    c = LA.adjoint_case(h, w)
    vjp = _vjp(eng, h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    fwd = eng.residual_lossy(c["u"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV), torch.zeros(1, 2, h, w, device=DEV))
    lhs = (fwd.cpu().double() * c["g"].double()).flatten(1).sum(1)
    rhs = (c["u"].double() * vjp.cpu().double()).flatten(1).sum(1)
    print(f"LOSSY ADJOINT {h}x{w} identity: " + ", ".join(f"{nm} <Au,g> {float(l):.6e} <u,A^H g> {float(r):.6e} |lhs-rhs| {abs(float(l - r)):.2e} bar "
                                                          f"{1e-5 * max(abs(float(l)), 1.0):.2e}" for nm, l, r in zip(LA.PROBES, lhs, rhs)))
    for l, r in zip(lhs.tolist(), rhs.tolist()):
        assert abs(l - r) <= 1e-5 * max(abs(l), 1.0), (l, r)


# ------------------------------------------------------------------------------------------------------------------------ 3: zero absorption
@pytest.mark.parametrize("n", [16, 48, 144, 256])
def test_zero_absorption_agrees_with_the_lossless_adjoint_and_two_calls_give_equal_bits(eng, n):
    c = LA.adjoint_case(n, n)
    eng.set_domain_rect(n, n, *R.DOMAIN)
    g, kq, ki = c["g"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV)
    a, b = eng.residual_vjp_lossy(g, kq, torch.zeros_like(ki)), eng.residual_vjp(g, kq)
    ratio = SP.peak(a.cpu().double() - b.cpu().double()) / (2 * LA.lossless_bar(c))
    print(f"LOSSY ADJOINT {n} k_sq_im = 0 against hn_residual_vjp: error / (2 bar) " + ", ".join(f"{float(r):.3f}" for r in ratio))
    assert bool((ratio <= 1.0).all()), ratio.tolist()
    assert torch.equal(eng.residual_vjp_lossy(g, kq, ki), _vjp(eng, n, n))
    eng.set_domain_rect(n, n, *R.DOMAIN)
    assert torch.equal(eng.residual_vjp_lossy(g, kq, ki), eng.residual_vjp_lossy(g, kq, ki))


# ------------------------------------------------------------------------------------------------------------------------------ 4: one cycle
def _cycle_problem(n, batch, rhs_batch, a0=0.1):
    s = _solver(n, (n // 2 - 2, n // 2))
    p = LA.ring_problem(n, a0, b=batch)
    src = s.source.detach().float().contiguous()
    if rhs_batch != 1:
        src = torch.cat([src * (1.0 + 0.5 * b) for b in range(rhs_batch)]).contiguous()
    return s, p["k_sq"].to(DEV), p["k_sq_im"].to(DEV), src


def _cyc(eng, adjoint, k_sq, k_im, rhs, restart, tol, m, alpha, x=None):
    b, n = k_sq.shape[0], k_sq.shape[-1]
    x = torch.zeros(b, 2, n, n, device=DEV) if x is None else x.clone()
    basis = torch.full((b, restart + 1, 2 * n * n), NAN, device=DEV)
    zbasis = torch.full((b, restart, 2 * n * n), NAN, device=DEV)
    hess = torch.full((b, restart + 1, restart, 2), NAN, device=DEV)
    if adjoint:
        rmse, k_used = eng.fgmres_adjoint_cycle_lossy(x, k_sq, k_im, rhs, restart, tol, m, alpha, basis=basis, zbasis=zbasis, hess=hess)
    else:
        rmse, k_used = eng.fgmres_cycle_lossy(x, k_sq, k_im, rhs, restart, tol, m, alpha, basis=basis, hess=hess, zbasis=zbasis)
    return {"x": x, "basis": basis, "zbasis": zbasis, "hess": hess, "rmse": rmse, "k_used": k_used}


_DENSE_UP_TO = 48      # the dense matrix of a sample: 85 MB at 48^2, 1.4 GB at 96^2
_DENSE = {}            # (n, checksums of the two planes) -> the dense float64 operator of that medium
_PIN = {}              # n -> the largest relative difference between the dense and the matrix-free float64 operator seen on the cycles' vectors


def _apply64(adjoint, rows, k_sq_b, k_im_b, n):
    """Rows of M v (or M^H v) for the complex rows v [m, P] in float64 on the host: by the dense M up to n = 48 (where the matrix-free operator of
    tests/lossy_common.py is applied too and the two are compared), matrix-free above."""
    free = _apply_free(adjoint, rows, k_sq_b, k_im_b, n)
    if n > _DENSE_UP_TO:
        return free
    key = (n, float(k_sq_b.double().sum()), float(k_im_b.double().sum()))      # the three ring media of a size: one matrix each
    if key not in _DENSE:
        _DENSE[key] = LA.lossy_matrix(k_sq_b[0].cpu().numpy(), k_im_b[0].cpu().numpy())
    M = _DENSE[key]
    dense = np.conj(np.conj(rows) @ M) if adjoint else rows @ M.T
    _PIN[n] = max(_PIN.get(n, 0.0), float(np.abs(dense - free).max() / np.abs(dense).max()))
    return dense


def _apply_free(adjoint, rows, k_sq_b, k_im_b, n):
    f = torch.from_numpy(np.stack([rows.real, rows.imag], 1).reshape(rows.shape[0], 2, n, n))
    kq, ki = k_sq_b.double().cpu()[None], k_im_b.double().cpu()[None]
    if adjoint:
        out = LA.adjoint_ref(f, kq, ki, n, n)
    else:
        with torch.no_grad():
            out = LC.residual(f, kq, ki, torch.zeros(1, 2, n, n, dtype=torch.float64), R.tables(n, n))
    return LA.np_complex(out)


def _iterates(Zc, Hc, beta, restart):
    out = []
    for j in range(1, restart + 1):
        e1 = np.zeros(j + 1, np.complex128); e1[0] = beta
        y = np.linalg.lstsq(Hc[: j + 1, :j], e1, rcond=None)[0]
        out.append((y[:, None] * Zc[:j]).sum(0))
    return np.stack(out)


def _invariants(run, adjoint, n, k_sq, k_im, rhs, restart):
    """(max |V^H V - I|, max |Op Z - V_{m+1} H| / max |H|, max_j |rmse[j] - true RMSE of the j-step iterate rebuilt in float64 from Z and H| / rmse[0])
    over the batch; the iterates start from x = 0."""
    orth = arn = dev = 0.0
    for b in range(k_sq.shape[0]):
        Vc, Zc = LA.np_complex(run["basis"][b]), LA.np_complex(run["zbasis"][b])
        Hc = run["hess"][b].double().cpu().numpy()
        Hc = Hc[..., 0] + 1j * Hc[..., 1]
        orth = max(orth, float(np.abs(Vc.conj() @ Vc.T - np.eye(restart + 1)).max()))
        arn = max(arn, float(np.abs(_apply64(adjoint, Zc, k_sq[b], k_im[b], n) - Hc.T @ Vc).max() / np.abs(Hc).max()))
        g = LA.np_complex(rhs[b if rhs.shape[0] > 1 else 0])
        beta = float(np.linalg.norm(g))
        res = g[None] - _apply64(adjoint, _iterates(Zc, Hc, beta, restart), k_sq[b], k_im[b], n)
        true = np.concatenate([[beta], np.linalg.norm(res, axis=1)]) / np.sqrt(2.0 * n * n)
        dev = max(dev, float(np.abs(run["rmse"][:, b].double().cpu().numpy() - true).max() / true[0]))
    return orth, arn, dev


@pytest.mark.parametrize("n,rhs_batch", [(48, 1), (48, 3), (96, 1), (96, 3)])
def test_arnoldi_invariants_of_one_plain_lossy_adjoint_cycle(n, rhs_batch):
    restart, batch = 5, 3
    s, k_sq, k_im, rhs = _cycle_problem(n, batch, rhs_batch)
    eng = s.engine()
    adj = _cyc(eng, True, k_sq, k_im, rhs, restart, 0.0, 0, 1.0)
    fwd = _cyc(eng, False, k_sq, k_im, rhs, restart, 0.0, 0, 1.0)
    assert adj["k_used"].tolist() == [restart] * batch
    for key in ("basis", "zbasis", "hess", "rmse"):
        assert bool(torch.isfinite(adj[key]).all()), key
    assert torch.equal(adj["zbasis"], adj["basis"][:, :restart])
    got = _invariants(adj, True, n, k_sq, k_im, rhs, restart)
    ref = _invariants(fwd, False, n, k_sq, k_im, rhs, restart)
    names = ("orthogonality", "arnoldi relation", "rmse estimate")
    for name, a, r in zip(names, got, ref):
        print(f"n={n} rhs_batch={rhs_batch} {name}: lossy adjoint {a:.3e}  lossy forward {r:.3e}  bar {4 * r:.3e}")
    for name, a, r in zip(names, got, ref):
        assert a <= 4 * r, (name, a, r)
    if n <= _DENSE_UP_TO:
        print(f"n={n}: dense M / M^H against the matrix-free float64 operator on the cycles' vectors: {_PIN[n]:.3e} of the largest entry, bar 1e-12")
        assert _PIN[n] <= 1e-12
    again = _cyc(eng, True, k_sq, k_im, rhs, restart, 0.0, 0, 1.0)
    for key in adj:
        assert torch.equal(adj[key], again[key]), key


def test_per_sample_stop_and_a_sample_that_starts_below_tol():
    from helmnet_amd.gmres import gmres_adjoint
    n, restart = 48, 8
    s, k_sq, k_im, rhs = _cycle_problem(n, 2, 2)
    eng = s.engine()
    full = _cyc(eng, True, k_sq, k_im, rhs, restart, 0.0, 0, 1.0)
    table = full["rmse"].cpu().numpy()
    print("rmse table", table.T.tolist())
    assert table[5, 0] < table[4, 0]
    tol = float(np.float32(np.sqrt(float(table[4, 0]) * float(table[5, 0]))))
    run = _cyc(eng, True, k_sq, k_im, rhs, restart, tol, 0, 1.0)
    ku = run["k_used"].tolist()
    want_ku = [int(np.nonzero(table[:, b] < tol)[0][0]) if (table[:, b] < tol).any() else restart for b in range(2)]
    print("tol", tol, "k_used", ku, "expected", want_ku)
    assert ku == want_ku and ku[0] == 5
    for key in ("basis", "zbasis", "hess"):
        assert torch.equal(run[key], full[key]), key
    rm = run["rmse"].cpu().numpy()
    for b in range(2):
        assert np.array_equal(rm[: ku[b] + 1, b], table[: ku[b] + 1, b]) and (rm[ku[b]:, b] == rm[ku[b], b]).all()
    # a sample that starts below tol is not written
    p = LA.ring_problem(n, 0.1, b=2)
    solved = gmres_adjoint(s, p["sos"][:1].to(DEV), rhs[:1], restart=40, max_outer=60, tol=1e-5, absorption=p["alpha"][:1].to(DEV))
    assert solved["converged"]
    x0 = torch.cat([solved["wavefield"], torch.zeros(1, 2, n, n, device=DEV)]).contiguous()
    run = _cyc(eng, True, k_sq, k_im, rhs, 4, 2e-5, 0, 1.0, x=x0)
    assert run["k_used"].tolist()[0] == 0 and run["k_used"].tolist()[1] > 0
    assert torch.equal(run["x"][0], x0[0]) and not torch.equal(run["x"][1], x0[1])
    assert bool((run["rmse"][:, 0] == run["rmse"][0, 0]).all()) and float(run["rmse"][0, 0]) < 2e-5


@pytest.mark.parametrize("m", [0, 2])
def test_one_cycle_at_256_lowers_the_true_residual(m):
    """restart 2, batch 1, a0 = 0.1 on the ring medium: the true residual rhs - A^H x (hn_residual_vjp_lossy) after the cycle is below the one at the
    start (row 0 of the table)."""
    n, restart = 256, 2
    s, k_sq, k_im, rhs = _cycle_problem(n, 1, 1)
    eng = s.engine()
    run = _cyc(eng, True, k_sq, k_im, rhs, restart, 0.0, m, _alpha_scale(rhs))
    for key in run:
        assert bool(torch.isfinite(run[key].float()).all()), key
    assert run["k_used"].tolist() == [restart]
    true = float((rhs - eng.residual_vjp_lossy(run["x"], k_sq, k_im)).double().pow(2).mean().sqrt())
    table = run["rmse"][:, 0].double().cpu().numpy()
    print(f"n=256 m={m}: rmse table {table.tolist()}, true rmse of the updated iterate {true:.6e}, start {table[0]:.6e}")
    assert true < table[0]
    if m == 0:
        assert torch.equal(run["zbasis"], run["basis"][:, :restart])


# -------------------------------------------------------------------------------------------------------------------------- 5: adjoint solve
@pytest.mark.parametrize("precondition", [None, "learned"])
@pytest.mark.parametrize("n,loc,a0", [(32, (12, 16), 0.1), (48, (14, 24), 0.02)])
def test_adjoint_solve_vs_float64_direct_solve(n, loc, a0, precondition):
    s = _solver(n, loc)
    p = LA.ring_problem(n, a0)
    g = LA.scaled_field((2, 2, n, n), 100 + n, float(torch.linalg.vector_norm(s.source.detach().double()))).to(DEV)
    out = s.adjoint_solve(g, p["sos"].to(DEV), precondition=precondition, restart=40, max_outer=60, tol=2e-6, precond_iterations=10,
                          absorption=p["alpha"].to(DEV))
    print(f"n={n} a0={a0} {precondition}: cycles {out['cycles']} iterations per sample {out['iterations_per_sample'].tolist()} converged "
          f"{out['converged']} true rmse {out['residual_norm'].tolist()} unet evaluations {out['unet_evaluations']}")
    assert out["converged"]
    got = LA.np_complex(out["wavefield"])
    for b in range(2):
        M = LA.lossy_matrix(p["k_sq"][b, 0].numpy(), p["k_sq_im"][b, 0].numpy())
        want = np.linalg.solve(M.conj().T, LA.np_complex(g[b]))
        err = max(np.abs(got[b].real - want.real).max(), np.abs(got[b].imag - want.imag).max())
        scale = max(np.abs(want.real).max(), np.abs(want.imag).max())
        print(f"n={n} a0={a0} {precondition} sample {b}: max|lam - lam64| = {err:.3e}, bar {2e-4 * scale:.3e}")
        assert err <= 2e-4 * scale, (b, err, scale)


# ---------------------------------------------------------------------------------------------------------------------- 6: pointwise kernel
@pytest.mark.parametrize("src_batch", [1, 3])
@pytest.mark.parametrize("n", [16, 48])
def test_adjoint_grad_lossy_kernel(eng, n, src_batch):
    eng.set_domain_rect(n, n, *R.DOMAIN)
    gen = torch.Generator().manual_seed(7 * n + src_batch)
    lam, u = (torch.randn(3, 2, n, n, generator=gen).to(DEV) for _ in range(2))
    g_k, g_ki, g_s = eng.adjoint_grad_lossy(lam, u, src_batch)
    old_k, old_s = eng.adjoint_grad(lam, u, src_batch)
    assert torch.equal(g_k, old_k) and torch.equal(g_s, old_s)                    # hn_adjoint_grad's, bit for bit
    again = eng.adjoint_grad_lossy(lam, u, src_batch)
    assert all(torch.equal(a, b) for a, b in zip((g_k, g_ki, g_s), again))
    ld, ud = lam.double(), u.double()
    want_k = -(ld * ud).sum(1, keepdim=True)
    want_ki = ld[:, 0:1] * ud[:, 1:2] - ld[:, 1:2] * ud[:, 0:1]
    bar = 4e-7 * float(lam.abs().max()) * float(u.abs().max())
    e_k, e_ki = float((g_k.double() - want_k).abs().max()), float((g_ki.double() - want_ki).abs().max())
    print(f"n={n} src_batch={src_batch}: max |g_k_sq - float64| = {e_k:.3e}, max |g_k_sq_im - float64| = {e_ki:.3e}, bar {bar:.3e}")
    assert tuple(g_k.shape) == tuple(g_ki.shape) == (3, 1, n, n) and e_k <= bar and e_ki <= bar
    assert torch.equal(g_s, lam if src_batch == 3 else ((lam[0] + lam[1]) + lam[2])[None])
    none = eng.adjoint_grad_lossy(lam, u, None)
    assert none[2] is None and torch.equal(none[0], g_k) and torch.equal(none[1], g_ki)
    # refusals leave the outputs alone
    keep = [t.clone() for t in (g_k, g_ki, g_s)]
    call = lambda l, uu, sb, b, gk, gki, gs: eng.lib.hn_adjoint_grad_lossy(eng.ctx, _p(l), _p(uu), sb, b, _p(gk), _p(gki), _p(gs), eng._stream())  # noqa: E731
    assert call(lam, u, 1, 3, g_k, 0, 0) == ERR_ARG and "NULL" in _err(eng)
    assert call(lam, 0, 1, 3, g_k, g_ki, 0) == ERR_ARG and "NULL" in _err(eng)
    assert call(lam, u, 1, 3, g_k, g_ki.data_ptr() + 4, 0) == ERR_ARG and "g_k_sq_im is not 16-byte aligned" in _err(eng)
    assert call(lam, u, 1, 3, g_k, g_k, 0) == ERR_ARG and "g_k_sq overlaps g_k_sq_im" in _err(eng)
    assert call(lam, u, 1, 3, g_k, lam, 0) == ERR_ARG and "overlaps" in _err(eng)
    assert call(lam, u, src_batch, 3, g_k, g_ki, g_ki.data_ptr() + 16) == ERR_ARG and "overlaps" in _err(eng)
    assert call(lam, u, 2, 3, g_k, g_ki, 0) == ERR_ARG and "src batch" in _err(eng)
    assert call(lam, u, 1, 0, g_k, g_ki, 0) == ERR_ARG and "batch" in _err(eng)
    eng.set_domain_rect(n, 2 * n, *R.DOMAIN)
    assert call(lam, u, 1, 3, g_k, g_ki, 0) == ERR_UNSUPPORTED and "rectangular domain" in _err(eng)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((g_k, g_ki, g_s), keep))


# ------------------------------------------------------------------------------------------------------------------ 7: gradients end to end
@pytest.mark.parametrize("n,loc", [(32, (12, 16)), (48, (14, 24))])
def test_implicit_gradients_vs_float64(n, loc):
    """solve_implicit(absorption = a tensor, tol 2e-6, restart 40, 60 cycles) + backward on the ring media with a0 = 0.1, the receiver-row loss of
    test_adjoint_gpu.test_implicit_gradient_vs_float64; sos.grad, alpha.grad and source.grad against the dense float64 adjoint-state values and a
    central difference (h 1e-6) of the float64 direct-solve loss: |<e, delta>| <= max|e| sum|delta| with the gradient's bar for max|e|."""
    a0 = 0.1
    s = _solver(n, loc)
    eng = s.engine()
    src = LA.np_complex(s.source.detach()[0])
    ref = LA.gradient_reference(n, a0, src)
    p = LA.ring_problem(n, a0)
    rx = ref["rx"]
    d = torch.from_numpy(np.stack([np.stack([x.real, x.imag]) for x in ref["d"]]).astype(np.float32)).to(DEV)      # [2, 2, n]
    sos = p["sos"].to(DEV).requires_grad_(True)
    alpha = p["alpha"].to(DEV).requires_grad_(True)
    s.source.requires_grad_(True)
    try:
        out = s.solve_implicit(sos, absorption=alpha, tol=2e-6, restart=40, max_cycles=60)
        u = out["wavefield"]
        assert u.requires_grad and out["converged"] and out["adjoint"] == {}
        loss = 0.5 * ((u[:, :, rx, :] - d) ** 2).sum()
        loss.backward()
        with pytest.raises(RuntimeError, match="create_graph"):
            out2 = s.solve_implicit(sos, absorption=alpha, tol=1e-3, restart=10, max_cycles=5)
            torch.autograd.grad(out2["wavefield"].sum(), sos, create_graph=True)
        g_sos, g_alpha = sos.grad.detach().double().cpu().numpy(), alpha.grad.detach().double().cpu().numpy()
        g_src = s.source.grad.detach().clone()
    finally:
        s.source.requires_grad_(False)
        s.source.grad = None
    info = out["adjoint"]
    print(f"n={n}: forward cycles {len(out['cycle_tables'])}, adjoint {info['cycles']} cycles, converged {info['converged']}, true rmse "
          f"{info['rmse'].tolist()}, unet evaluations {info['unet_evaluations']}")
    assert info["converged"] and float(info["rmse"].max()) < 2e-6
    # dJ/dk_sq and dJ/dk_sq_im by the same two calls backward makes: the adjoint solve of the loss's cotangent, then hn_adjoint_grad_lossy
    cot = torch.zeros_like(u.detach()); cot[:, :, rx, :] = u.detach()[:, :, rx, :] - d
    lam = s.adjoint_solve(cot.contiguous(), sos.detach(), restart=40, max_outer=60, tol=2e-6, precondition="learned", absorption=alpha.detach())["wavefield"]
    g_k, g_ki, _ = (t if t is None else t.double().cpu().numpy() for t in eng.adjoint_grad_lossy(lam, u.detach().contiguous(), None))
    src_bar = 0.0
    for b in range(2):
        ml = max(np.abs(ref["lam"][b].real).max(), np.abs(ref["lam"][b].imag).max())
        mu = max(np.abs(ref["u"][b].real).max(), np.abs(ref["u"][b].imag).max())
        base = 4e-4 * ml * mu
        errs = {"g_k_sq": (np.abs(g_k[b, 0] - ref["g_k_sq"][b]).max(), base), "g_k_sq_im": (np.abs(g_ki[b, 0] - ref["g_k_sq_im"][b]).max(), base),
                "sos.grad": (np.abs(g_sos[b, 0] - ref["g_sos"][b]).max(), base * ref["chain_sos"][b]),
                "alpha.grad": (np.abs(g_alpha[b, 0] - ref["g_alpha"][b]).max(), base * ref["chain_alpha"][b])}
        print(f"n={n} sample {b}: max|lam| {ml:.3e} max|u| {mu:.3e}; " + "; ".join(f"{k} error {e:.3e}, bar {bar:.3e}" for k, (e, bar) in errs.items()))
        for k, (e, bar) in errs.items():
            assert e <= bar, (k, e, bar)
        src_bar += 2e-4 * ml
        sb, ab = p["sos"][b, 0].double().numpy(), p["alpha"][b, 0].double().numpy()
        for name, grad, chain, moved in (("sos", g_sos, ref["chain_sos"][b], 0), ("alpha", g_alpha, ref["chain_alpha"][b], 1)):
            delta = np.random.default_rng(300 + n + b + 10 * moved).standard_normal((n, n))
            h = 1e-6
            plus = (sb + h * delta, ab) if moved == 0 else (sb, ab + h * delta)
            minus = (sb - h * delta, ab) if moved == 0 else (sb, ab - h * delta)
            fd = (LA.loss64(ref["M"][b], sb, ab, *plus, src, rx, ref["d"][b]) - LA.loss64(ref["M"][b], sb, ab, *minus, src, rx, ref["d"][b])) / (2 * h)
            an = float((grad[b, 0] * delta).sum())
            bar = base * chain * float(np.abs(delta).sum())
            print(f"n={n} sample {b}: <{name}.grad, delta> {an:.8e}  central difference {fd:.8e}  difference {abs(an - fd):.3e}, bar {bar:.3e}")
            assert abs(an - fd) <= bar
    got_src = LA.np_complex(g_src[0])
    e = max(np.abs(got_src.real - ref["g_src"].reshape(-1).real).max(), np.abs(got_src.imag - ref["g_src"].reshape(-1).imag).max())
    print(f"n={n}: source.grad error {e:.3e}, bar {src_bar:.3e}")
    assert tuple(g_src.shape) == (1, 2, n, n) and e <= src_bar


def test_a_number_for_absorption_runs_and_gets_no_gradient():
    """n = 32, absorption = 0.1 as a Python number (alpha = 0.1 everywhere): sos.grad against the dense float64 values of that medium, at its bar."""
    n, loc, a0 = 32, (12, 16), 0.1
    s = _solver(n, loc)
    src = LA.np_complex(s.source.detach()[0])
    ref = LA.gradient_reference(n, a0, src, uniform=True)
    p = LA.ring_problem(n, a0, uniform=True)
    rx = ref["rx"]
    d = torch.from_numpy(np.stack([np.stack([x.real, x.imag]) for x in ref["d"]]).astype(np.float32)).to(DEV)
    sos = p["sos"].to(DEV).requires_grad_(True)
    out = s.solve_implicit(sos, absorption=a0, tol=2e-6, restart=40, max_cycles=60)
    (0.5 * ((out["wavefield"][:, :, rx, :] - d) ** 2).sum()).backward()
    assert out["converged"] and out["adjoint"]["converged"] and s.source.grad is None
    g_sos = sos.grad.detach().double().cpu().numpy()
    for b in range(2):
        ml = max(np.abs(ref["lam"][b].real).max(), np.abs(ref["lam"][b].imag).max())
        mu = max(np.abs(ref["u"][b].real).max(), np.abs(ref["u"][b].imag).max())
        e, bar = np.abs(g_sos[b, 0] - ref["g_sos"][b]).max(), 4e-4 * ml * mu * ref["chain_sos"][b]
        print(f"n={n} absorption={a0} sample {b}: sos.grad error {e:.3e}, bar {bar:.3e}")
        assert e <= bar
    # a tensor with one value per sample receives the sum over the dimensions it broadcasts along
    per = torch.tensor([a0, a0], device=DEV).reshape(2, 1, 1, 1).requires_grad_(True)
    sos2 = p["sos"].to(DEV).requires_grad_(True)
    out = s.solve_implicit(sos2, absorption=per, tol=2e-6, restart=40, max_cycles=60)
    (0.5 * ((out["wavefield"][:, :, rx, :] - d) ** 2).sum()).backward()
    assert tuple(per.grad.shape) == (2, 1, 1, 1)
    for b in range(2):
        ml = max(np.abs(ref["lam"][b].real).max(), np.abs(ref["lam"][b].imag).max())
        mu = max(np.abs(ref["u"][b].real).max(), np.abs(ref["u"][b].imag).max())
        want = float(ref["g_alpha"][b].sum())
        e, bar = abs(float(per.grad[b]) - want), 4e-4 * ml * mu * ref["chain_alpha"][b] * n * n
        print(f"n={n} one alpha per sample, sample {b}: grad {float(per.grad[b]):.6e} float64 {want:.6e} error {e:.3e}, bar {bar:.3e} (n^2 entries summed)")
        assert e <= bar


# ---------------------------------------------------------------------------------------------------------------------- 8: refusals and order
def _raw_cycle(eng, x, k_sq, k_im, rhs, rhs_batch, batch, restart, tol, m, alpha, basis, zbasis, hess, rmse, k_used):
    return eng.lib.hn_fgmres_adjoint_cycle_lossy(eng.ctx, _p(x), _p(k_sq), _p(k_im), _p(rhs), rhs_batch, batch, restart, tol, m, alpha, _p(basis),
                                                 _p(zbasis), _p(hess), _p(rmse), _p(k_used), eng._stream())


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
    c = LA.adjoint_case(h, w)
    g, kq, ki = c["g"].to(DEV), c["k_sq"].to(DEV), c["k_sq_im"].to(DEV)
    out = torch.full_like(g, NAN)
    vjp = lambda g_, kq_, ki_, out_, b: eng.lib.hn_residual_vjp_lossy(eng.ctx, _p(g_), _p(kq_), _p(ki_), _p(out_), b, eng._stream())  # noqa: E731
    assert vjp(g, kq, 0, out, 3) == ERR_ARG and "hn_residual_vjp)" in _err(eng) and "k_sq_im is NULL" in _err(eng)
    assert vjp(g, 0, ki, out, 3) == ERR_ARG and "NULL" in _err(eng)
    assert vjp(g, kq, ki, out, 0) == ERR_ARG and "batch" in _err(eng)
    assert vjp(g, kq, ki, g, 3) == ERR_ARG and "alias" in _err(eng)
    assert vjp(g, kq, out.data_ptr() + 64, out, 1) == ERR_ARG and "k_sq_im overlaps out" in _err(eng)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the cycle: NULL k_sq_im names the lossless sibling; a rectangular domain is unsupported
    bufs = _buffers(h, w, 3, 4)
    x, basis, zbasis, hess, rmse, k_used = bufs
    rhs = torch.zeros(1, 2, h, w, device=DEV)
    assert _raw_cycle(eng, x, kq, 0, rhs, 1, 3, 4, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used) == ERR_ARG and "hn_fgmres_adjoint_cycle)" in _err(eng)
    assert _raw_cycle(eng, x, kq, ki, rhs, 1, 3, 4, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used) == ERR_UNSUPPORTED
    assert "rectangular domain" in _err(eng) and "hn_fgmres_adjoint_cycle_lossy" in _err(eng)
    _left_alone(bufs)
    # on a square domain: k_sq_im by k_sq's rules
    n = 32
    eng.set_domain_rect(n, n, *R.DOMAIN)
    bufs = _buffers(n, n, 2, 3)
    x, basis, zbasis, hess, rmse, k_used = bufs
    kq, ki, rhs = torch.ones(2, 1, n, n, device=DEV), torch.zeros(2, 1, n, n, device=DEV), torch.zeros(1, 2, n, n, device=DEV)
    call = lambda **kw: _raw_cycle(eng, **{**dict(x=x, k_sq=kq, k_im=ki, rhs=rhs, rhs_batch=1, batch=2, restart=3, tol=0.0, m=0, alpha=1.0, basis=basis,  # noqa: E731
                                                  zbasis=zbasis, hess=hess, rmse=rmse, k_used=k_used), **kw})
    assert call(k_im=ki.data_ptr() + 4) == ERR_ARG and "k_sq_im is not 16-byte aligned" in _err(eng)
    assert call(k_im=kq) == ERR_ARG and "k_sq_im overlaps k_sq" in _err(eng)
    assert call(k_im=basis) == ERR_ARG and "k_sq_im overlaps basis" in _err(eng)
    assert call(restart=0) == ERR_ARG and "restart" in _err(eng)
    assert call(m=-1) == ERR_ARG and "precond_iters" in _err(eng)
    assert call(zbasis=0) == ERR_ARG and "NULL" in _err(eng)
    _left_alone(bufs)
    with pytest.raises(RuntimeError, match="grad"):
        eng.fgmres_adjoint_cycle_lossy(x, kq, ki.clone().requires_grad_(True), rhs, 3, 0.0, 0, 1.0)


def test_first_lossy_adjoint_call_under_stream_capture_is_refused_and_the_capture_ends_clean():
    n = 64
    e = _engine()
    e.set_domain_rect(n, n, *R.DOMAIN)          # a power of two: the lossless routes build no line tables
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(2, 2, n, n, generator=gen).to(DEV)
    kq, ki = R.seeded_k_sq(n, n, 2, 1).to(DEV), LC.seeded_k_sq_im(n, n, 2, 2).to(DEV)
    out = torch.full_like(g, NAN)
    probe = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probe.add_(1.0)
        rc = e.lib.hn_residual_vjp_lossy(e.ctx, _p(g), _p(kq), _p(ki), _p(out), 2, e._stream())
        msg = _err(e)
    assert rc == ERR_STATE and "captur" in msg and "hn_residual_vjp_lossy" in msg
    graph.replay()                                # the capture is still valid, and holds nothing of the library's
    torch.cuda.synchronize()
    assert probe.tolist() == [1.0] * 4 and bool(torch.isnan(out).all())
    got = e.residual_vjp_lossy(g, kq, ki)         # eager: builds the tables
    other = _engine()                             # a context that was never refused
    other.set_domain_rect(n, n, *R.DOMAIN)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, other.residual_vjp_lossy(g, kq, ki))
    for x in (e, other):
        torch.cuda.synchronize()
        x.check_async_errors()
        x.close()


# ------------------------------------------------------------------------------------------------------------------- 9: nothing else moved
def _lossless_family(e, n, case):
    """hn_residual, hn_residual_vjp, hn_residual_lossy, two hn_step iterations and one hn_fgmres_adjoint_cycle on seeded inputs."""
    u, kq, ki, src = case
    out = {"residual": e.residual(u, kq, src), "vjp": e.residual_vjp(u, kq), "lossy": e.residual_lossy(u, kq, ki, src)}
    wf, res = torch.zeros_like(u), e.residual(torch.zeros_like(u), kq, src)
    st = torch.zeros(u.shape[0], 2, R.state_len(n, n), device=DEV)
    e.step(wf, res, st, kq, src, 2)
    out.update(step_wf=wf, step_res=res, step_states=st)
    x = torch.zeros_like(u)
    basis, zbasis = torch.zeros(u.shape[0], 4, 2 * n * n, device=DEV), torch.zeros(u.shape[0], 3, 2 * n * n, device=DEV)
    hess = torch.zeros(u.shape[0], 4, 3, 2, device=DEV)
    rmse, k_used = e.fgmres_adjoint_cycle(x, kq, src, 3, 0.0, 2, _alpha_scale(src), basis=basis, zbasis=zbasis, hess=hess)
    out.update(x=x, basis=basis, zbasis=zbasis, hess=hess, rmse=rmse, k_used=k_used)
    torch.cuda.synchronize()
    e.check_async_errors()
    return out


@pytest.mark.parametrize("n", [64, 96, 144])
def test_the_lossless_family_and_the_forward_lossy_operator_are_untouched(blob, n):
    """A context that has run the three new calls against a fresh one, bit for bit: 64 (radix-4), 96 (prime-factor) and 144, the mixed route that
    shares its axis tables and the <., true> instances with the lossy adjoint."""
    gen = torch.Generator().manual_seed(n)
    u = torch.randn(2, 2, n, n, generator=gen).to(DEV)
    kq, ki = R.seeded_k_sq(n, n, 2, 10 + n).to(DEV), LC.seeded_k_sq_im(n, n, 2, 20 + n).to(DEV)
    src = R.point_source_map(n, n, [n // 4, n // 2], 10.0).to(DEV).contiguous()
    case = (u, kq, ki, src)
    fresh, used = _engine(blob), _engine(blob)
    for e in (fresh, used):
        e.set_domain_rect(n, n, *R.DOMAIN)
    g = used.residual_vjp_lossy(u, kq, ki)
    run = _cyc(used, True, kq, ki, src, 3, 0.0, 2, _alpha_scale(src))
    used.adjoint_grad_lossy(run["x"], g, 1)
    torch.cuda.synchronize()
    used.check_async_errors()
    assert bool(torch.isfinite(run["x"]).all())
    a, b = _lossless_family(fresh, n, case), _lossless_family(used, n, case)
    for key in a:
        assert bool(torch.isfinite(a[key].float()).all()), key
        assert torch.equal(a[key], b[key]), key
    fresh.close()
    used.close()
