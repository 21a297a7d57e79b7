"""hn_gmres_cycle on the GPU: the solve against a float64 direct solve, the Arnoldi invariants of one cycle against the torch backend's own
arithmetic, the residual history against float64 GMRES, bit-reproducibility, the per-sample stop, the driver, and the refusals.

Where a bar is "k times what backend='torch' shows", the torch figure comes from ``_torch_cycle``: the parent's Arnoldi loop (gmres.py: ``project``,
the chunked basis, the host Givens solve) re-run on the same inputs with its basis and Hessenberg matrix kept.  Every figure is printed before it
is asserted (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import helmnet_oracle as O

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
_SOLVERS = {}


def _solver(n, loc=None):
    from helmnet_amd import IterativeSolver
    if n not in _SOLVERS:
        s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
        s.set_domain_size(n, source_location=loc if loc is not None else [n // 2 - 2, n // 2])
        _SOLVERS[n] = s
    return _SOLVERS[n]


@pytest.fixture(autouse=True)
def _async_errors_clean():
    yield
    torch.cuda.synchronize()
    for s in _SOLVERS.values():
        s.engine().check_async_errors()


def _problem(n, batch, rhs_batch=1, seed=None):
    from helmnet_amd.phantoms import ring_sos_batch
    s = _solver(n)
    sos = torch.from_numpy(ring_sos_batch(n, batch, seed=n if seed is None else seed)).to(DEV)
    k_sq = s.get_initials(sos)[0].contiguous()
    src = s.source.detach().float().contiguous()
    if rhs_batch != 1:
        src = torch.cat([src * (1.0 + 0.5 * b) for b in range(rhs_batch)]).contiguous()
    return s, k_sq, src


def _cycle(eng, k_sq, rhs, restart, tol, x=None):
    b, n = k_sq.shape[0], k_sq.shape[-1]
    x = torch.zeros(b, 2, n, n, device=DEV) if x is None else x.clone()
    basis = torch.full((b, restart + 1, 2 * n * n), float("nan"), device=DEV)
    hess = torch.full((b, restart + 1, restart, 2), float("nan"), device=DEV)
    rmse, k_used = eng.gmres_cycle(x, k_sq, rhs, restart, tol, basis, hess)
    return {"x": x, "basis": basis, "hess": hess, "rmse": rmse, "k_used": k_used}


def _torch_cycle(eng, k_sq, rhs, restart):
    """The parent's cycle from x = 0 (gmres.py, backend='torch'), keeping V and H: basis [B, m + 1, 2 n^2], hess [B, m + 1, m, 2], rmse [m + 1, B] and
    the fp32 update of every truncation k as a function."""
    from helmnet_amd.gmres import _back_substitute, _hessenberg_least_squares
    bsz, n = k_sq.shape[0], k_sq.shape[-1]
    P2 = 2 * n * n
    c = 512 if P2 % 512 == 0 else P2
    S = P2 // c
    zero_src = torch.zeros(1, 2, n, n, device=DEV)
    b_f = rhs.expand(bsz, -1, -1, -1).contiguous().reshape(bsz, P2)

    def apply_a(v):
        return eng.residual(v.reshape(bsz, 2, n, n).contiguous(), k_sq, zero_src).reshape(bsz, P2)

    def rot(v):
        return torch.cat([-v[:, P2 // 2:], v[:, : P2 // 2]], 1)

    V = torch.empty(bsz, S, restart + 1, c, device=DEV)
    H = torch.zeros(bsz, restart + 1, restart, 2, device=DEV)

    def project(w, k):
        Vk = V[:, :, : k + 1].reshape(bsz * S, k + 1, c)
        W2 = torch.stack([w, -rot(w)], -1).reshape(bsz * S, c, 2)
        h = torch.bmm(Vk, W2).reshape(bsz, S, k + 1, 2).sum(1)
        hh = h.unsqueeze(1).expand(bsz, S, k + 1, 2).reshape(bsz * S, k + 1, 2)
        ab = torch.bmm(Vk.transpose(1, 2), hh).reshape(bsz, P2, 2)
        return h, w - ab[..., 0] - rot(ab[..., 1])

    x = torch.zeros(bsz, P2, device=DEV)
    r = b_f - apply_a(x)
    beta = torch.linalg.vector_norm(r, dim=1)
    V[:, :, 0] = (r / beta.clamp_min(1e-30).unsqueeze(1)).reshape(bsz, S, c)
    for k in range(restart):
        w = apply_a(V[:, :, k].reshape(bsz, P2))
        h, w = project(w, k)
        h2, w = project(w, k)
        hn = torch.linalg.vector_norm(w, dim=1)
        H[:, : k + 1, k] = h + h2
        H[:, k + 1, k, 0] = hn
        V[:, :, k + 1] = (w / hn.clamp_min(1e-30).unsqueeze(1)).reshape(bsz, S, c)
    beta_h = beta.double().cpu().numpy()
    Hh = H.double().cpu().numpy()
    R, g, res = _hessenberg_least_squares(Hh[..., 0] + 1j * Hh[..., 1], beta_h)
    rm = np.concatenate([beta_h[:, None], res], 1) / np.sqrt(float(P2))
    basis = V.permute(0, 2, 1, 3).reshape(bsz, restart + 1, P2).contiguous()

    def update(b, k):   # the parent's fp32 update of sample b truncated at k steps
        y = _back_substitute(R[b:b + 1], g[b:b + 1], k)[0]
        yy = torch.from_numpy(np.stack([y.real, y.imag], -1).astype(np.float32)).to(DEV)
        ab = basis[b, :k].t() @ yy
        return (ab[:, 0] + rot(ab[None, :, 1])[0]).reshape(2, n, n)

    return {"basis": basis, "hess": H, "rmse": torch.from_numpy(rm.T.astype(np.float32)).to(DEV), "update": update}


def _complex(v):   # [..., 2 P] planar -> complex128 [..., P]
    p = v.shape[-1] // 2
    return torch.complex(v[..., :p].double(), v[..., p:].double())


def _apply64(eng, fields, k_sq_b, src64):
    """A v (src64 zero) or A v - src for a stack of fields [m, 2, n, n] float64 of ONE sample's k_sq [1, 1, n, n]."""
    m = fields.shape[0]
    return eng.residual64(fields.contiguous(), k_sq_b.double().expand(m, -1, -1, -1).contiguous(), src64, True, False)[0]


def _lstsq_iterates(eng, basis_b, hess_b, rhs_b, restart):
    """The j-step GMRES iterates (j = 1 .. restart) of one sample rebuilt in float64 from its basis and Hessenberg matrix: [restart, 2, n, n]."""
    n = rhs_b.shape[-1]
    Vc = _complex(basis_b).cpu().numpy()                       # [m + 1, P]
    Hc = hess_b.double().cpu().numpy()
    Hc = Hc[..., 0] + 1j * Hc[..., 1]
    beta = float(torch.linalg.vector_norm(rhs_b.double()))
    out = []
    for j in range(1, restart + 1):
        e1 = np.zeros(j + 1, np.complex128); e1[0] = beta
        y = np.linalg.lstsq(Hc[: j + 1, :j], e1, rcond=None)[0]
        xj = (y[:, None] * Vc[:j]).sum(0)
        out.append(np.stack([xj.real, xj.imag]).reshape(2, n, n))
    return torch.from_numpy(np.stack(out)).to(DEV), beta


def _invariants(eng, run, k_sq, rhs, restart):
    """(max |V^H V - I|, max |A V_m - V_{m+1} H| / max |H|, max_j |rmse[j] - true RMSE of the j-step float64 iterate| / rmse[0]) over the batch."""
    bsz, n = k_sq.shape[0], k_sq.shape[-1]
    zero64 = torch.zeros(1, 2, n, n, device=DEV, dtype=torch.float64)
    orth = arn = dev = 0.0
    for b in range(bsz):
        rhs_b = rhs[b if rhs.shape[0] > 1 else 0]
        Vc = _complex(run["basis"][b])                                                # [m + 1, P]
        Hc = torch.complex(run["hess"][b, ..., 0].double(), run["hess"][b, ..., 1].double())   # [m + 1, m]
        gram = Vc.conj() @ Vc.t()
        orth = max(orth, float((gram - torch.eye(restart + 1, device=DEV, dtype=gram.dtype)).abs().max()))
        AV = _apply64(eng, run["basis"][b, :restart].double().reshape(restart, 2, n, n), k_sq[b:b + 1], zero64)
        AVc = _complex(AV.reshape(restart, -1))                                       # rows: A v_k
        arn = max(arn, float((AVc - Hc.t() @ Vc).abs().max() / Hc.abs().max()))
        its, beta = _lstsq_iterates(eng, run["basis"][b], run["hess"][b], rhs_b, restart)
        res = _apply64(eng, its, k_sq[b:b + 1], rhs_b.double().unsqueeze(0).contiguous())
        true = torch.cat([torch.tensor([beta / np.sqrt(2.0 * n * n)], device=DEV, dtype=torch.float64), res.pow(2).mean((1, 2, 3)).sqrt()])
        dev = max(dev, float((run["rmse"][:, b].double() - true).abs().max() / true[0]))
    return orth, arn, dev


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n,loc", [(32, [12, 16]), (48, [14, 24])])
def test_hip_gmres_vs_float64_direct_solve(n, loc):
    from helmnet_amd import IterativeSolver
    from helmnet_amd.gmres import gmres
    from helmnet_amd.phantoms import ring_sos_batch
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
    s.set_domain_size(n, source_location=loc)
    sos = ring_sos_batch(n, 2, seed=n)
    out = gmres(s, torch.from_numpy(sos).to(DEV), restart=40, max_outer=60, tol=2e-6, backend="hip")
    got = out["wavefield"].cpu().numpy()
    src = s.source.detach().cpu().numpy()[0]
    print("iterations per sample", out["iterations_per_sample"].tolist(), "converged", out["converged"])
    for b in range(2):
        want = O.direct_solve(sos[b, 0], src, 8, 2.0, 1.0)
        err, scale = np.abs(got[b] - want).max(), np.abs(want).max()
        print(f"n={n} sample {b}: max|got - want| = {err:.3e}, bar {2e-4 * scale:.3e}")
        assert err <= 2e-4 * scale, (b, err, scale)
    s.engine().check_async_errors()


# ---------------------------------------------------------------------------------------------- 2
_GRID = [(16, 5, 3, 1), (48, 5, 3, 1), (96, 5, 3, 1), (144, 5, 3, 1), (16, 1, 3, 1), (16, 64, 3, 1), (48, 5, 3, 3)]


@pytest.mark.parametrize("n,restart,batch,rhs_batch", _GRID)
def test_arnoldi_invariants_of_one_cycle(n, restart, batch, rhs_batch):
    """Bars: 4 x what the torch backend's arithmetic shows on the same inputs (the summation order differs, both are fp32)."""
    s, k_sq, rhs = _problem(n, batch, rhs_batch)
    eng = s.engine()
    hip = _cycle(eng, k_sq, rhs, restart, 0.0)
    assert hip["k_used"].tolist() == [restart] * batch
    assert bool(torch.isfinite(hip["basis"]).all()) and bool(torch.isfinite(hip["hess"]).all()) and bool(torch.isfinite(hip["rmse"]).all())
    got = _invariants(eng, hip, k_sq, rhs, restart)
    ref = _invariants(eng, _torch_cycle(eng, k_sq, rhs, restart), k_sq, rhs, restart)
    for name, g, r in zip(("orthogonality", "arnoldi relation", "rmse estimate"), got, ref):
        print(f"n={n} restart={restart} rhs_batch={rhs_batch} {name}: hip {g:.3e}  torch {r:.3e}  bar {4 * r:.3e}")
    for name, g, r in zip(("orthogonality", "arnoldi relation", "rmse estimate"), got, ref):
        assert g <= 4 * r, (name, g, r)


# ---------------------------------------------------------------------------------------------- 3
def test_residual_history_vs_float64_gmres():
    n, restart = 32, 20
    s, k_sq, rhs = _problem(n, 2)
    eng = s.engine()
    hip = _cycle(eng, k_sq, rhs, restart, 0.0)["rmse"].double().cpu().numpy()
    tor = _torch_cycle(eng, k_sq, rhs, restart)["rmse"].double().cpu().numpy()
    src = rhs[0].double().cpu().numpy()
    b0 = (src[0] + 1j * src[1]).reshape(-1)
    for b in range(2):
        M = O.assemble_helmholtz_matrix(k_sq[b, 0].double().cpu().numpy(), 8, 2.0, 1.0)
        beta = np.linalg.norm(b0)
        Q = np.zeros((restart + 1, b0.size), np.complex128)
        H = np.zeros((restart + 1, restart), np.complex128)
        Q[0] = b0 / beta
        want = []
        for k in range(restart):
            w = M @ Q[k]
            for _ in range(2):
                h = Q[: k + 1].conj() @ w
                w = w - h @ Q[: k + 1]
                H[: k + 1, k] += h
            H[k + 1, k] = np.linalg.norm(w)
            Q[k + 1] = w / H[k + 1, k]
            e1 = np.zeros(k + 2, np.complex128); e1[0] = beta
            y = np.linalg.lstsq(H[: k + 2, : k + 1], e1, rcond=None)[0]
            want.append(np.linalg.norm(e1 - H[: k + 2, : k + 1] @ y) / np.sqrt(2.0 * n * n))
        want = np.array(want)
        d_hip = (np.abs(hip[1:, b] - want) / want).max()
        d_tor = (np.abs(tor[1:, b] - want) / want).max()
        print(f"sample {b}: relative deviation from float64 GMRES: hip {d_hip:.3e}  torch {d_tor:.3e}  bar {2 * d_tor:.3e}")
        assert d_hip <= 2 * d_tor, (b, d_hip, d_tor)


# ---------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n", [48, 96])
def test_determinism_and_batch_independence(n):
    s, k_sq, rhs = _problem(n, 3)
    eng = s.engine()
    a = _cycle(eng, k_sq, rhs, 6, 0.0)
    b = _cycle(eng, k_sq, rhs, 6, 0.0)
    for key in ("x", "basis", "hess", "rmse", "k_used"):
        assert torch.equal(a[key], b[key]), key
    solo = _cycle(eng, k_sq[1:2].contiguous(), rhs, 6, 0.0)
    for key in ("x", "basis", "hess", "k_used"):
        assert torch.equal(a[key][1], solo[key][0]), key
    assert torch.equal(a["rmse"][:, 1], solo["rmse"][:, 0])


def _fresh_engine(key):
    from helmnet_amd.engine import Engine
    eng = Engine(torch.device(DEV))
    eng.set_domain(16, *key[1:])
    eng.set_domain(*key)                           # a fresh domain: no GMRES workspace yet
    return eng


def test_workspace_grown_then_reused_by_a_smaller_call():
    """Small, large, small again on one context: the workspace is built for (1, 3), grown to (3, 6), then to (3, 9) -- the batch shrinks, the restart
    grows: each keeps its own maximum -- and a (1, 3) call in a workspace sized for more gives the bits of the (1, 3) call that built it.
    n = 48: three 1024-pixel chunks per sample, the last one partial, so the strides of the partial-sum table matter."""
    n = 48
    s, k_sq, rhs = _problem(n, 3)
    eng, other = _fresh_engine(s.engine().domain_key), _fresh_engine(s.engine().domain_key)
    one, two = k_sq[:1].contiguous(), k_sq[:2].contiguous()
    first = _cycle(eng, one, rhs, 3, 0.0)
    big = _cycle(eng, k_sq, rhs, 6, 0.0)
    mid = _cycle(eng, two, rhs, 9, 0.0)
    last = _cycle(eng, one, rhs, 3, 0.0)
    assert first["k_used"].tolist() == [3] and big["k_used"].tolist() == [6] * 3 and mid["k_used"].tolist() == [9] * 2
    for key in ("x", "basis", "hess", "rmse", "k_used"):
        assert torch.equal(first[key], last[key]), key
    solo = _cycle(other, one, rhs, 6, 0.0)         # a context that has only ever seen this call
    for key in ("x", "basis", "hess", "k_used"):
        assert torch.equal(big[key][0], solo[key][0]), key
    assert torch.equal(big["rmse"][:, 0], solo["rmse"][:, 0])
    for e in (eng, other):
        torch.cuda.synchronize()
        e.check_async_errors()
        e.close()


# ---------------------------------------------------------------------------------------------- 5
def test_per_sample_stop_sample_below_tol_is_untouched():
    from helmnet_amd.gmres import gmres
    from helmnet_amd.phantoms import ring_sos_batch
    n, restart = 32, 12
    s, k_sq, rhs = _problem(n, 2)
    eng = s.engine()
    sos = torch.from_numpy(ring_sos_batch(n, 2, seed=n)).to(DEV)
    solved = gmres(s, sos[:1], restart=40, max_outer=60, tol=1e-5, backend="hip")
    assert solved["converged"]
    x0 = torch.cat([solved["wavefield"], torch.zeros(1, 2, n, n, device=DEV)]).contiguous()
    run = _cycle(eng, k_sq, rhs, restart, 2e-5, x=x0)
    assert int(run["k_used"][0]) == 0
    assert torch.equal(run["x"][0], x0[0])
    assert bool((run["rmse"][:, 0] == run["rmse"][0, 0]).all()) and float(run["rmse"][0, 0]) < 2e-5
    solo = _cycle(eng, k_sq[1:2].contiguous(), rhs, restart, 2e-5)
    for key in ("x", "basis", "hess", "k_used"):
        assert torch.equal(run[key][1], solo[key][0]), key
    assert torch.equal(run["rmse"][:, 1], solo["rmse"][:, 0])


def test_per_sample_stop_mid_cycle_uses_that_truncation():
    n, restart = 32, 20
    s, k_sq, rhs = _problem(n, 2)
    eng = s.engine()
    full = _cycle(eng, k_sq, rhs, restart, 0.0)
    table = full["rmse"].cpu().numpy()
    assert table[10, 0] < table[9, 0]
    tol = float(np.sqrt(float(table[9, 0]) * float(table[10, 0])))
    run = _cycle(eng, k_sq, rhs, restart, tol)
    ku = run["k_used"].tolist()
    want_ku = [int(np.nonzero(table[:, b] < tol)[0][0]) if (table[:, b] < tol).any() else restart for b in range(2)]
    print("tol", tol, "k_used", ku)
    assert ku == want_ku and ku[0] == 10
    assert torch.equal(run["basis"], full["basis"]) and torch.equal(run["hess"], full["hess"])     # the lock-step work goes on
    rm = run["rmse"].cpu().numpy()
    for b in range(2):
        assert np.array_equal(rm[: ku[b] + 1, b], table[: ku[b] + 1, b]) and (rm[ku[b]:, b] == rm[ku[b], b]).all()
    tor = _torch_cycle(eng, k_sq, rhs, restart)
    for b in range(2):
        k = ku[b]
        want, _ = _lstsq_iterates(eng, run["basis"][b], run["hess"][b], rhs[0], restart)
        want_t, _ = _lstsq_iterates(eng, tor["basis"][b], tor["hess"][b], rhs[0], restart)
        d_hip = float((run["x"][b].double() - want[k - 1]).abs().max() / want[k - 1].abs().max())
        d_tor = float((tor["update"](b, k).double() - want_t[k - 1]).abs().max() / want_t[k - 1].abs().max())
        print(f"sample {b}, k_used {k}: |x - float64 lstsq iterate| / max: hip {d_hip:.3e}  torch {d_tor:.3e}  bar {4 * d_tor:.3e}")
        assert d_hip <= 4 * d_tor, (b, d_hip, d_tor)


# ---------------------------------------------------------------------------------------------- 6
def test_driver_parity_with_torch_backend_and_learned_start():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.gmres import gmres
    from helmnet_amd.phantoms import ring_sos_batch
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
    s.set_domain_size(96, source_location=[82, 48])
    eng = s.engine()
    sos = torch.from_numpy(ring_sos_batch(96, 2, seed=11)).to(DEV)
    k_sq = s.get_initials(sos)[0].contiguous()
    # unpreconditioned GMRES(30) needs some hundred cycles here (the torch run below is cut off after 40, as in the test this set-up comes from)
    hip = gmres(s, sos, restart=30, max_outer=600, tol=2e-4, backend="hip")
    print("hip: cycles", len(hip["cycle_tables"]), "lock-step iterations", hip["iterations"], "last", hip["residual_norms"][-1].tolist())
    assert hip["converged"] and hip["iterations_per_sample"].dtype == torch.int64 and hip["iterations_per_sample"].shape == (2,)
    true_rmse = eng.rmse(s.get_residual(hip["wavefield"], k_sq))
    print("hip: final", hip["residual_norms"][-1].tolist(), "true", true_rmse.tolist(), "iterations", hip["iterations_per_sample"].tolist())
    assert torch.allclose(true_rmse, hip["residual_norms"][-1].to(true_rmse.device), rtol=5e-2, atol=2e-5)
    assert float(true_rmse.max()) < 2e-4
    tor = gmres(s, sos, restart=30, max_outer=40, tol=2e-4)
    a, b = hip["wavefield"], tor["wavefield"]
    rel = (a - b).abs().amax(dim=(1, 2, 3)) / b.abs().amax(dim=(1, 2, 3))
    print("hip vs torch wavefield, relative to max:", rel.tolist())
    assert float(rel.max()) < 0.05, rel
    learned = s.forward(sos, num_iterations=100, residuals="norms")["wavefields"][0].contiguous()
    keep = learned.clone()
    start = eng.rmse(s.get_residual(learned, k_sq))
    cont = s.gmres(sos, restart=30, max_cycles=600, tol=2e-4, x0=learned)
    first = cont["residual_norms"][0]
    print("learned start: hn_rmse", start.tolist(), "history[0]", first.tolist(), "cycles", len(cont["cycle_tables"]))
    assert torch.allclose(first, start, rtol=1e-5, atol=0)
    assert cont["converged"] and torch.equal(learned, keep)   # x0 is not written
    for table in cont["cycle_tables"]:
        assert (np.diff(table, axis=0) <= 0).all()
    eng.check_async_errors()


# ---------------------------------------------------------------------------------------------- 7
def _raw(eng, x, k_sq, rhs, rhs_batch, batch, restart, tol, basis, hess, rmse, k_used):
    p = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    return eng.lib.hn_gmres_cycle(eng.ctx, p(x), p(k_sq), p(rhs), rhs_batch, batch, restart, tol, p(basis), p(hess), p(rmse), p(k_used), eng._stream())


def _buffers(n, batch, restart):
    return (torch.zeros(batch, 2, n, n, device=DEV), torch.empty(batch, restart + 1, 2 * n * n, device=DEV), torch.empty(batch, restart + 1, restart, 2, device=DEV),
            torch.empty(restart + 1, batch, device=DEV), torch.empty(batch, device=DEV, dtype=torch.int32))


def test_argument_refusals():
    n = 32
    s, k_sq, rhs = _problem(n, 3)
    eng = s.engine()
    x, basis, hess, rmse, k_used = _buffers(n, 3, 4)
    err = lambda: eng.lib.hn_last_error(eng.ctx).decode()  # noqa: E731
    assert _raw(eng, x, k_sq, rhs, 1, 3, 4, 0.0, x, hess, rmse, k_used) == -1 and "overlaps" in err()
    assert _raw(eng, x, k_sq, rhs, 1, 3, 4, 0.0, x.data_ptr() + 16, hess, rmse, k_used) == -1 and "overlaps" in err()
    assert _raw(eng, x, k_sq, k_sq, 1, 3, 4, 0.0, basis, hess, rmse, k_used) == -1 and "k_sq overlaps rhs" in err()      # read against read
    assert _raw(eng, x, k_sq, rhs, 1, 3, 0, 0.0, basis, hess, rmse, k_used) == -1 and "restart" in err()
    assert _raw(eng, x, k_sq, rhs, 1, 3, 65, 0.0, basis, hess, rmse, k_used) == -1 and "restart" in err()
    assert _raw(eng, x, k_sq, rhs, 2, 3, 4, 0.0, basis, hess, rmse, k_used) == -1 and "rhs batch" in err()
    assert _raw(eng, x, k_sq, rhs, 1, 0, 4, 0.0, basis, hess, rmse, k_used) == -1 and "batch" in err()
    assert _raw(eng, x, k_sq, rhs, 1, 3, 4, 0.0, 0, hess, rmse, k_used) == -1 and "NULL" in err()
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0                                    # nothing ran
    with pytest.raises(RuntimeError, match="grad"):
        eng.gmres_cycle(x, k_sq.clone().requires_grad_(True), rhs, 4, 0.0)
    with pytest.raises(ValueError):
        eng.gmres_cycle(x, k_sq, rhs, 4, 0.0, basis=basis[:, :4])


def _hip_runtime():
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the HIP runtime is not mapped")


def test_stream_capture_first_call_refused_then_replays_to_the_same_bits():
    from helmnet_amd.engine import Engine
    n, restart, batch = 32, 6, 2
    s, k_sq, rhs = _problem(n, batch)
    eng = Engine(torch.device(DEV))                # a fresh context: no GMRES workspace yet
    eng.set_domain(*s.engine().domain_key)
    x, basis, hess, rmse, k_used = _buffers(n, batch, restart)
    basis.fill_(-7.0)
    probe = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        probe.add_(1.0)
        rc = _raw(eng, x, k_sq, rhs, 1, batch, restart, 0.0, basis, hess, rmse, k_used)
    assert rc == -2 and "capture" in eng.lib.hn_last_error(eng.ctx).decode()
    g.replay()                                     # the capture is still valid, and holds nothing of the library's
    torch.cuda.synchronize()
    assert probe.tolist() == [1.0] * 4 and float(x.abs().max()) == 0.0 and bool((basis == -7.0).all())
    assert _raw(eng, x, k_sq, rhs, 1, batch, restart, 0.0, basis, hess, rmse, k_used) == 0      # eager: builds the workspace
    torch.cuda.synchronize()
    want = [t.clone() for t in (x, basis, hess, rmse, k_used)]
    assert want[4].tolist() == [restart] * batch
    # captured by hand on a side stream, so that the graph's shape can be read: one root, a linear chain
    hip = _hip_runtime()
    side = torch.cuda.Stream()
    graph, count, edges = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
    x.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        st = ctypes.c_void_p(side.cuda_stream)
        assert hip.hipStreamBeginCapture(st, 1) == 0           # hipStreamCaptureModeThreadLocal
        rc = _raw(eng, x, k_sq, rhs, 1, batch, restart, 0.0, basis, hess, rmse, k_used)
        assert hip.hipStreamEndCapture(st, ctypes.byref(graph)) == 0
    assert rc == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(count)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(edges)) == 0
    roots = ctypes.c_size_t()
    assert hip.hipGraphGetRootNodes(graph, None, ctypes.byref(roots)) == 0
    print("captured cycle:", count.value, "nodes,", edges.value, "edges,", roots.value, "root")
    assert roots.value == 1 and count.value >= 5 * restart + 5 and edges.value == count.value - 1
    exe = ctypes.c_void_p()
    assert hip.hipGraphInstantiate(ctypes.byref(exe), graph, None, None, 0) == 0
    for t in (basis, hess, rmse):
        t.fill_(float("nan"))
    k_used.fill_(-1)
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(exe, ctypes.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    for got, ref, name in zip((x, basis, hess, rmse, k_used), want, ("x", "basis", "hess", "rmse", "k_used")):
        assert torch.equal(got, ref), name
    assert hip.hipGraphExecDestroy(exe) == 0 and hip.hipGraphDestroy(graph) == 0
    eng.check_async_errors()
    eng.close()
