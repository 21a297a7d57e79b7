"""hn_fgmres_cycle / hn_fgmres_refine_cycle on the GPU: without a preconditioner they are the GMRES entry points bit for bit; the z_j are the public
``step`` composed as the header says, bit for bit; the flexible Arnoldi relation A Z = V H, the orthogonality of V and the residual estimate against
a torch restatement of the same cycle; the update over Z; bit-reproducibility; the refusals; and the preconditioned refinement at 96^2.

Where a bar is "4 x the torch restatement", the figure comes from ``_torch_fcycle``: the torch backend's Arnoldi arithmetic (gmres.py: ``project``, the
chunked basis, the host Givens solve) with z_k = M(v_k) by ``Engine.step`` and w = A z_k.  Every figure is printed before it is asserted (pytest -s).
The helpers of tests/test_gmres_gpu.py are used as they are."""
import ctypes

import numpy as np
import pytest
import torch

import test_gmres_gpu as G

DEV = G.DEV
pytestmark = pytest.mark.gpu
_FP16 = {}
_KEYS = ("x", "basis", "zbasis", "hess", "rmse", "k_used")


@pytest.fixture(autouse=True)
def _async_errors_clean():
    yield
    torch.cuda.synchronize()
    for s in list(G._SOLVERS.values()) + list(_FP16.values()):
        s.engine().check_async_errors()


def _new_solver(n, precision=None):
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
    if precision is not None:
        s.set_unet_precision(precision)
    s.set_domain_size(n, source_location=[n // 2 - 2, n // 2])
    return s


def _alpha(rhs):
    from helmnet_amd.gmres import default_precond_scale
    return float(np.float32(default_precond_scale(rhs)))      # (the C interface takes it as a float)


def _fcycle(eng, k_sq, rhs, restart, tol, m, alpha, x=None):
    b, n = k_sq.shape[0], k_sq.shape[-1]
    x = torch.zeros(b, 2, n, n, device=DEV) if x is None else x.clone()
    basis = torch.full((b, restart + 1, 2 * n * n), float("nan"), device=DEV)
    zbasis = torch.full((b, restart, 2 * n * n), float("nan"), device=DEV)
    hess = torch.full((b, restart + 1, restart, 2), float("nan"), device=DEV)
    rmse, k_used = eng.fgmres_cycle(x, k_sq, rhs, restart, tol, m, alpha, basis, hess, zbasis)
    return {"x": x, "basis": basis, "zbasis": zbasis, "hess": hess, "rmse": rmse, "k_used": k_used}


def _precond(eng, k_sq, v, m, alpha):
    """M(v) for v [B, 2 n^2] by the public calls, as the header composes it: src = alpha v, zeros, res = 0 - src, ``step`` m times, wf / alpha (the
    scalar as a device tensor: a true division, not a multiplication by the reciprocal)."""
    b, n = k_sq.shape[0], k_sq.shape[-1]
    a = torch.tensor(alpha, dtype=torch.float32, device=DEV)
    src = (a * v).reshape(b, 2, n, n).contiguous()
    wf = torch.zeros_like(src)
    res = torch.zeros_like(src) - src
    states = torch.zeros(b, 2, eng.state_len, device=DEV)
    eng.step(wf, res, states, k_sq, src, m)
    return (wf / a).reshape(b, 2 * n * n)


def _torch_fcycle(eng, k_sq, rhs, restart, m, alpha):
    """``test_gmres_gpu._torch_cycle`` as a flexible cycle from x = 0: basis, zbasis, hess, rmse and the fp32 update of every truncation."""
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
    Z = torch.empty(bsz, restart, P2, device=DEV)
    H = torch.zeros(bsz, restart + 1, restart, 2, device=DEV)

    def project(w, k):
        Vk = V[:, :, : k + 1].reshape(bsz * S, k + 1, c)
        W2 = torch.stack([w, -rot(w)], -1).reshape(bsz * S, c, 2)
        h = torch.bmm(Vk, W2).reshape(bsz, S, k + 1, 2).sum(1)
        hh = h.unsqueeze(1).expand(bsz, S, k + 1, 2).reshape(bsz * S, k + 1, 2)
        ab = torch.bmm(Vk.transpose(1, 2), hh).reshape(bsz, P2, 2)
        return h, w - ab[..., 0] - rot(ab[..., 1])

    r = b_f - apply_a(torch.zeros(bsz, P2, device=DEV))
    beta = torch.linalg.vector_norm(r, dim=1)
    V[:, :, 0] = (r / beta.clamp_min(1e-30).unsqueeze(1)).reshape(bsz, S, c)
    for k in range(restart):
        Z[:, k] = _precond(eng, k_sq, V[:, :, k].reshape(bsz, P2), m, alpha)
        w = apply_a(Z[:, k])
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

    def update(b, k):   # the fp32 update of sample b truncated at k steps, over Z
        y = _back_substitute(R[b:b + 1], g[b:b + 1], k)[0]
        yy = torch.from_numpy(np.stack([y.real, y.imag], -1).astype(np.float32)).to(DEV)
        ab = Z[b, :k].t() @ yy
        return (ab[:, 0] + rot(ab[None, :, 1])[0]).reshape(2, n, n)

    return {"basis": basis, "zbasis": Z, "hess": H, "rmse": torch.from_numpy(rm.T.astype(np.float32)).to(DEV), "update": update}


def _lstsq_iterates(zbasis_b, hess_b, rhs_b, restart):
    """The j-step FGMRES iterates (j = 1 .. restart) of one sample from x = 0, rebuilt in float64 from Z and H: [restart, 2, n, n]."""
    n = rhs_b.shape[-1]
    Zc = G._complex(zbasis_b).cpu().numpy()                      # [m, P]
    Hc = hess_b.double().cpu().numpy()
    Hc = Hc[..., 0] + 1j * Hc[..., 1]
    beta = float(torch.linalg.vector_norm(rhs_b.double()))
    out = []
    for j in range(1, restart + 1):
        e1 = np.zeros(j + 1, np.complex128); e1[0] = beta
        y = np.linalg.lstsq(Hc[: j + 1, :j], e1, rcond=None)[0]
        xj = (y[:, None] * Zc[:j]).sum(0)
        out.append(np.stack([xj.real, xj.imag]).reshape(2, n, n))
    return torch.from_numpy(np.stack(out)).to(DEV), beta


def _invariants(eng, run, k_sq, rhs, restart):
    """(max |V^H V - I|, max |A Z_m - V_{m+1} H| / max |H|, max_j |rmse[j] - true RMSE of the j-step float64 iterate from Z and H| / rmse[0])."""
    bsz, n = k_sq.shape[0], k_sq.shape[-1]
    zero64 = torch.zeros(1, 2, n, n, device=DEV, dtype=torch.float64)
    orth = arn = dev = 0.0
    for b in range(bsz):
        rhs_b = rhs[b if rhs.shape[0] > 1 else 0]
        Vc = G._complex(run["basis"][b])
        Hc = torch.complex(run["hess"][b, ..., 0].double(), run["hess"][b, ..., 1].double())
        gram = Vc.conj() @ Vc.t()
        orth = max(orth, float((gram - torch.eye(restart + 1, device=DEV, dtype=gram.dtype)).abs().max()))
        AZ = G._apply64(eng, run["zbasis"][b].double().reshape(restart, 2, n, n), k_sq[b:b + 1], zero64)
        arn = max(arn, float((G._complex(AZ.reshape(restart, -1)) - Hc.t() @ Vc).abs().max() / Hc.abs().max()))
        its, beta = _lstsq_iterates(run["zbasis"][b], run["hess"][b], rhs_b, restart)
        res = G._apply64(eng, its, k_sq[b:b + 1], rhs_b.double().unsqueeze(0).contiguous())
        true = torch.cat([torch.tensor([beta / np.sqrt(2.0 * n * n)], device=DEV, dtype=torch.float64), res.pow(2).mean((1, 2, 3)).sqrt()])
        dev = max(dev, float((run["rmse"][:, b].double() - true).abs().max() / true[0]))
    return orth, arn, dev


# ---------------------------------------------------------------------------------------------- 1
_PLAIN = [(32, 5, 3, 1), (48, 64, 2, 2), (16, 1, 1, 1)]


@pytest.mark.parametrize("n,restart,batch,rhs_batch", _PLAIN)
def test_without_preconditioner_the_cycle_is_hn_gmres_cycle_bit_for_bit(n, restart, batch, rhs_batch):
    s, k_sq, rhs = G._problem(n, batch, rhs_batch)
    eng = s.engine()
    want = G._cycle(eng, k_sq, rhs, restart, 0.0)
    got = _fcycle(eng, k_sq, rhs, restart, 0.0, 0, _alpha(rhs))
    for key in ("x", "basis", "hess", "rmse", "k_used"):
        assert torch.equal(got[key], want[key]), key
    assert torch.equal(got["zbasis"], want["basis"][:, :restart])
    assert got["k_used"].tolist() == [restart] * batch


@pytest.mark.parametrize("n,restart,batch,rhs_batch", _PLAIN)
def test_without_preconditioner_the_refinement_is_hn_gmres_refine_cycle_bit_for_bit(n, restart, batch, rhs_batch):
    s, k_sq, rhs = G._problem(n, batch, rhs_batch)
    eng = s.engine()
    x0 = (0.01 * torch.randn(batch, 2, n, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)).to(DEV)
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    xa, ba, ha = x0.clone(), new(batch, restart + 1, 2 * n * n), new(batch, restart + 1, restart, 2)
    r64a, rma, kua = eng.gmres_refine_cycle(xa, k_sq, rhs, restart, 1e-10, 1e-6, ba, ha)
    xb, bb, hb, zb = x0.clone(), new(batch, restart + 1, 2 * n * n), new(batch, restart + 1, restart, 2), new(batch, restart, 2 * n * n)
    r64b, rmb, kub = eng.fgmres_refine_cycle(xb, k_sq, rhs, restart, 1e-10, 0, _alpha(rhs), 1e-6, bb, hb, zb)
    for a, b, name in ((xa, xb, "x"), (ba, bb, "basis"), (ha, hb, "hess"), (r64a, r64b, "rmse64"), (rma, rmb, "rmse"), (kua, kub, "k_used")):
        assert torch.equal(a, b), name
    assert torch.equal(zb, ba[:, :restart])
    assert not torch.equal(xa, x0)


# ---------------------------------------------------------------------------------------------- 2
# 256: the smallest size at which the hand-scheduled level-0 kernels and the multi-workgroup deep kernel run; they need an aligned batch of 1
@pytest.mark.parametrize("n,restart,batch,m", [(32, 4, 2, 1), (32, 4, 2, 3), (256, 2, 1, 2)])
def test_z_is_the_public_step_composed_as_the_header_says(n, restart, batch, m):
    s, k_sq, rhs = G._problem(n, batch)
    eng = s.engine()
    alpha = _alpha(rhs)
    run = _fcycle(eng, k_sq, rhs, restart, 0.0, m, alpha)
    assert bool(torch.isfinite(run["zbasis"]).all()) and run["k_used"].tolist() == [restart] * batch
    for j in range(restart):
        want = _precond(eng, k_sq, run["basis"][:, j].contiguous(), m, alpha)
        assert torch.equal(run["zbasis"][:, j], want), j
        assert float(want.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- 3
def _check_invariants(s, k_sq, rhs, restart, batch, m, tag):
    eng = s.engine()
    alpha = _alpha(rhs)
    hip = _fcycle(eng, k_sq, rhs, restart, 0.0, m, alpha)
    assert hip["k_used"].tolist() == [restart] * batch
    for key in ("basis", "zbasis", "hess", "rmse"):
        assert bool(torch.isfinite(hip[key]).all()), key
    got = _invariants(eng, hip, k_sq, rhs, restart)
    ref = _invariants(eng, _torch_fcycle(eng, k_sq, rhs, restart, m, alpha), k_sq, rhs, restart)
    names = ("orthogonality", "flexible arnoldi relation", "rmse estimate")
    for name, g, r in zip(names, got, ref):
        print(f"{tag} restart={restart} m={m} {name}: hip {g:.3e}  torch {r:.3e}  bar {4 * r:.3e}")
    for name, g, r in zip(names, got, ref):
        assert g <= 4 * r, (name, g, r)


@pytest.mark.parametrize("n,restart,batch,rhs_batch,m", [(32, 5, 3, 1, 2), (48, 5, 3, 3, 1), (96, 8, 2, 1, 3)])
def test_flexible_arnoldi_invariants_of_one_cycle(n, restart, batch, rhs_batch, m):
    """Bars: 4 x what the torch restatement of the same flexible cycle shows on the same inputs (the summation order differs, both are fp32)."""
    s, k_sq, rhs = G._problem(n, batch, rhs_batch)
    _check_invariants(s, k_sq, rhs, restart, batch, m, f"n={n} rhs_batch={rhs_batch}")


@pytest.mark.parametrize("n,restart,batch,m", [(32, 5, 3, 2), (128, 4, 2, 2)])
def test_flexible_arnoldi_invariants_hold_for_the_fp16_network_too(n, restart, batch, m):
    """The bars do not depend on what the preconditioner is: the first case again on a solver of its own whose UNet runs in fp16.  The 16-bit kernels
    serve the levels that are at least 128 wide (hn_mfma.hip: launch_dc_mfma, launch_down, launch_up); below that the fp16 mode runs the fp32
    kernels and the z_j are the fp32 ones bit for bit.  So the case is also run at 128^2, the smallest size at which the preconditioner really is
    another one: there the z_j must differ."""
    if n not in _FP16:
        _FP16[n] = _new_solver(n, "fp16")
    s = _FP16[n]
    assert s.engine().unet_precision == "fp16"
    s32, k_sq, rhs = G._problem(n, batch, 1)
    assert s32.engine().unet_precision == "fp32"
    _check_invariants(s, k_sq, rhs, restart, batch, m, f"n={n} fp16")
    alpha = _alpha(rhs)
    z16 = _fcycle(s.engine(), k_sq, rhs, restart, 0.0, m, alpha)["zbasis"]
    z32 = _fcycle(s32.engine(), k_sq, rhs, restart, 0.0, m, alpha)["zbasis"]
    diff = float((z16 - z32).abs().max() / z32.abs().max())
    print(f"n={n}: max |z(fp16) - z(fp32)| / max |z| = {diff:.3e}")
    assert (diff > 0.0) == (n >= 128)


# ---------------------------------------------------------------------------------------------- 4
def test_update_is_the_sum_over_z_at_each_samples_own_truncation():
    """Two sources of different strength, a tolerance between rows 4 and 5 of sample 0's table: the samples stop at their own k, and x - 0 is
    sum_{j < k_used} y_j z_j with y from a float64 least-squares solve on hess.  Bar: 4 x the torch restatement's own deviation."""
    n, restart, m = 32, 8, 2
    s, k_sq, rhs = G._problem(n, 2, 2)
    eng = s.engine()
    alpha = _alpha(rhs)
    full = _fcycle(eng, k_sq, rhs, restart, 0.0, m, alpha)
    table = full["rmse"].cpu().numpy()
    print("rmse table", table.T.tolist())
    assert table[5, 0] < table[4, 0]
    tol = float(np.float32(np.sqrt(float(table[4, 0]) * float(table[5, 0]))))
    run = _fcycle(eng, k_sq, rhs, restart, tol, m, alpha)
    ku = run["k_used"].tolist()
    want_ku = [int(np.nonzero(table[:, b] < tol)[0][0]) if (table[:, b] < tol).any() else restart for b in range(2)]
    print("tol", tol, "k_used", ku)
    assert ku == want_ku and ku[0] == 5 and ku[1] != ku[0]
    for key in ("basis", "zbasis", "hess"):                        # the lock-step work goes on
        assert torch.equal(run[key], full[key]), key
    rm = run["rmse"].cpu().numpy()
    for b in range(2):
        assert np.array_equal(rm[: ku[b] + 1, b], table[: ku[b] + 1, b]) and (rm[ku[b]:, b] == rm[ku[b], b]).all()
    tor = _torch_fcycle(eng, k_sq, rhs, restart, m, alpha)
    for b in range(2):
        k = ku[b]
        want, _ = _lstsq_iterates(run["zbasis"][b], run["hess"][b], rhs[b], restart)
        want_t, _ = _lstsq_iterates(tor["zbasis"][b], tor["hess"][b], rhs[b], restart)
        d_hip = float((run["x"][b].double() - want[k - 1]).abs().max() / want[k - 1].abs().max())
        d_tor = float((tor["update"](b, k).double() - want_t[k - 1]).abs().max() / want_t[k - 1].abs().max())
        print(f"sample {b}, k_used {k}: |x - float64 lstsq iterate over Z| / max: hip {d_hip:.3e}  torch {d_tor:.3e}  bar {4 * d_tor:.3e}")
        assert d_hip <= 4 * d_tor, (b, d_hip, d_tor)


def test_sample_that_starts_below_tol_is_untouched():
    from helmnet_amd.gmres import gmres
    from helmnet_amd.phantoms import ring_sos_batch
    n, restart, m = 32, 4, 2
    s, k_sq, rhs = G._problem(n, 2)
    eng = s.engine()
    sos = torch.from_numpy(ring_sos_batch(n, 2, seed=n)).to(DEV)
    solved = gmres(s, sos[:1], restart=40, max_outer=60, tol=1e-5, backend="hip")
    assert solved["converged"]
    x0 = torch.cat([solved["wavefield"], torch.zeros(1, 2, n, n, device=DEV)]).contiguous()
    run = _fcycle(eng, k_sq, rhs, restart, 2e-5, m, _alpha(rhs), x=x0)
    assert run["k_used"].tolist()[0] == 0 and run["k_used"].tolist()[1] > 0
    assert torch.equal(run["x"][0], x0[0]) and not torch.equal(run["x"][1], x0[1])
    assert bool((run["rmse"][:, 0] == run["rmse"][0, 0]).all()) and float(run["rmse"][0, 0]) < 2e-5


# ---------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("n", [48, 96])
def test_two_calls_give_equal_bits_and_a_broadcast_rhs_equals_explicit_copies(n):
    s, k_sq, rhs = G._problem(n, 3)
    eng = s.engine()
    alpha = _alpha(rhs)
    a = _fcycle(eng, k_sq, rhs, 4, 0.0, 2, alpha)
    b = _fcycle(eng, k_sq, rhs, 4, 0.0, 2, alpha)
    c = _fcycle(eng, k_sq, rhs.expand(3, -1, -1, -1).contiguous(), 4, 0.0, 2, alpha)
    for key in _KEYS:
        assert bool(torch.isfinite(a[key].float()).all()), key
        assert torch.equal(a[key], b[key]), key
        assert torch.equal(a[key], c[key]), key


# ---------------------------------------------------------------------------------------------- 6
def _p(t):
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _raw(eng, x, k_sq, rhs, rhs_batch, batch, restart, tol, m, alpha, basis, zbasis, hess, rmse, k_used):
    return eng.lib.hn_fgmres_cycle(eng.ctx, _p(x), _p(k_sq), _p(rhs), rhs_batch, batch, restart, tol, m, alpha, _p(basis), _p(zbasis), _p(hess), _p(rmse),
                                   _p(k_used), eng._stream())


def _raw_refine(eng, x, k_sq, rhs, rhs_batch, batch, restart, tol, floor, m, alpha, basis, zbasis, hess, rmse, k_used, rmse64):
    return eng.lib.hn_fgmres_refine_cycle(eng.ctx, _p(x), _p(k_sq), _p(rhs), rhs_batch, batch, restart, tol, floor, m, alpha, _p(basis), _p(zbasis),
                                          _p(hess), _p(rmse), _p(k_used), _p(rmse64), eng._stream())


def _buffers(n, batch, restart, dtype=torch.float32):
    """x, basis, zbasis, hess, rmse, k_used: x zero, the others -7 so that a refused call is seen to have left them alone."""
    f = lambda *shape: torch.full(shape, -7.0, device=DEV)  # noqa: E731
    return (torch.zeros(batch, 2, n, n, device=DEV, dtype=dtype), f(batch, restart + 1, 2 * n * n), f(batch, restart, 2 * n * n),
            f(batch, restart + 1, restart, 2), f(restart + 1, batch), torch.full((batch,), -7, device=DEV, dtype=torch.int32))


def _left_alone(bufs):
    torch.cuda.synchronize()
    assert float(bufs[0].abs().max()) == 0.0
    for t in bufs[1:]:
        assert bool((t == -7).all())


def test_argument_refusals_leave_the_outputs_alone():
    n = 32
    s, k_sq, rhs = G._problem(n, 3)
    eng = s.engine()
    bufs = _buffers(n, 3, 4)
    x, basis, zbasis, hess, rmse, k_used = bufs
    err = lambda: eng.lib.hn_last_error(eng.ctx).decode()  # noqa: E731
    call = lambda **kw: _raw(eng, **{**dict(x=x, k_sq=k_sq, rhs=rhs, rhs_batch=1, batch=3, restart=4, tol=0.0, m=1, alpha=1.0, basis=basis,  # noqa: E731
                                            zbasis=zbasis, hess=hess, rmse=rmse, k_used=k_used), **kw})
    # what hn_gmres_cycle refuses
    assert call(basis=x) == -1 and "overlaps" in err()
    assert call(rhs=k_sq) == -1 and "k_sq overlaps rhs" in err()
    assert call(restart=0) == -1 and "restart" in err()
    assert call(restart=65) == -1 and "restart" in err()
    assert call(rhs_batch=2) == -1 and "rhs batch" in err()
    assert call(batch=0) == -1 and "batch" in err()
    assert call(basis=0) == -1 and "NULL" in err()
    assert call(basis=basis.data_ptr() + 4) == -1 and "aligned" in err()
    # the preconditioner's own
    assert call(m=-1) == -1 and "precond_iters" in err()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(alpha=bad) == -1 and "precond_scale" in err(), bad
    assert call(zbasis=0) == -1 and "NULL" in err()
    assert call(zbasis=zbasis.data_ptr() + 4) == -1 and "zbasis is not 16-byte aligned" in err()
    assert call(zbasis=basis) == -1 and "basis overlaps zbasis" in err()
    assert call(zbasis=x) == -1 and "x overlaps zbasis" in err()
    assert call(zbasis=basis.data_ptr() + 16 * 2 * n * n) == -1 and "overlaps" in err()
    assert call(m=0, alpha=0.0) == -1 and "precond_scale" in err()                   # refused whatever m is
    _left_alone(bufs)
    # the refinement: the same, and its tolerances
    bufs64 = _buffers(n, 3, 4, torch.float64)
    x64 = bufs64[0]
    rmse64 = torch.full((3,), -7.0, device=DEV, dtype=torch.float64)
    rcall = lambda **kw: _raw_refine(eng, **{**dict(x=x64, k_sq=k_sq, rhs=rhs, rhs_batch=1, batch=3, restart=4, tol=1e-10, floor=1e-6, m=1, alpha=1.0,  # noqa: E731
                                                    basis=bufs64[1], zbasis=bufs64[2], hess=bufs64[3], rmse=bufs64[4], k_used=bufs64[5], rmse64=rmse64), **kw})
    assert rcall(tol=float("nan")) == -1 and "tol" in err()
    assert rcall(floor=-1.0) == -1 and "inner_floor" in err()
    assert rcall(m=-2) == -1 and "precond_iters" in err()
    assert rcall(alpha=float("inf")) == -1 and "precond_scale" in err()
    assert rcall(zbasis=0) == -1 and "NULL" in err()
    assert rcall(zbasis=x64) == -1 and "x overlaps zbasis" in err()
    assert rcall(rmse64=0) == -1 and "NULL" in err()
    _left_alone(bufs64 + (rmse64,))
    with pytest.raises(RuntimeError, match="grad"):
        eng.fgmres_cycle(x, k_sq.clone().requires_grad_(True), rhs, 4, 0.0, 1, 1.0)
    with pytest.raises(ValueError):
        eng.fgmres_cycle(x, k_sq, rhs, 4, 0.0, 1, 1.0, zbasis=basis)                 # restart + 1 slots: not a zbasis


def test_state_refusals_no_domain_and_no_weights():
    from helmnet_amd.engine import Engine
    n = 32
    s, k_sq, rhs = G._problem(n, 2)
    bufs = _buffers(n, 2, 3)
    x, basis, zbasis, hess, rmse, k_used = bufs
    rmse64 = torch.full((2,), -7.0, device=DEV, dtype=torch.float64)
    x64 = torch.zeros(2, 2, n, n, device=DEV, dtype=torch.float64)
    eng = Engine(torch.device(DEV))                # a fresh context: no domain, no weights
    err = lambda: eng.lib.hn_last_error(eng.ctx).decode()  # noqa: E731
    assert _raw(eng, x, k_sq, rhs, 1, 2, 3, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used) == -2 and "hn_set_domain" in err()
    assert _raw_refine(eng, x64, k_sq, rhs, 1, 2, 3, 1e-10, 1e-6, 0, 1.0, basis, zbasis, hess, rmse, k_used, rmse64) == -2 and "hn_set_domain" in err()
    eng.set_domain(*s.engine().domain_key)
    assert _raw(eng, x, k_sq, rhs, 1, 2, 3, 0.0, 1, 1.0, basis, zbasis, hess, rmse, k_used) == -2 and "hn_load_weights" in err()
    assert _raw_refine(eng, x64, k_sq, rhs, 1, 2, 3, 1e-10, 1e-6, 2, 1.0, basis, zbasis, hess, rmse, k_used, rmse64) == -2 and "hn_load_weights" in err()
    _left_alone(bufs + (rmse64,))
    assert float(x64.abs().max()) == 0.0
    # without a preconditioner the network is not needed
    assert _raw(eng, x, k_sq, rhs, 1, 2, 3, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used) == 0
    want = G._cycle(s.engine(), k_sq, rhs, 3, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(x, want["x"]) and torch.equal(zbasis, want["basis"][:, :3])
    eng.check_async_errors()
    eng.close()


def test_workspace_grown_by_a_larger_batch_then_reused_by_a_smaller_call():
    n, restart, m = 48, 3, 2
    _, k_sq, rhs = G._problem(n, 3)
    s = _new_solver(n)                             # a context of its own: no preconditioner workspace yet
    eng = s.engine()
    alpha = _alpha(rhs)
    one = k_sq[:1].contiguous()
    first = _fcycle(eng, one, rhs, restart, 0.0, m, alpha)
    big = _fcycle(eng, k_sq, rhs, restart, 0.0, m, alpha)
    last = _fcycle(eng, one, rhs, restart, 0.0, m, alpha)
    assert first["k_used"].tolist() == [restart] and big["k_used"].tolist() == [restart] * 3
    for key in _KEYS:
        assert bool(torch.isfinite(big[key].float()).all()), key
        assert torch.equal(first[key], last[key]), key
    want = _precond(eng, k_sq, big["basis"][:, 1].contiguous(), m, alpha)      # the grown workspace serves every sample
    assert torch.equal(big["zbasis"][:, 1], want)
    torch.cuda.synchronize()
    eng.check_async_errors()


def test_first_call_under_stream_capture_is_refused_and_the_capture_ends_clean():
    n, restart, batch = 32, 3, 2
    _, k_sq, rhs = G._problem(n, batch)
    s = _new_solver(n)
    eng = s.engine()
    bufs = _buffers(n, batch, restart)
    x, basis, zbasis, hess, rmse, k_used = bufs
    x64 = torch.zeros(batch, 2, n, n, device=DEV, dtype=torch.float64)
    rmse64 = torch.full((batch,), -7.0, device=DEV, dtype=torch.float64)
    probe = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        probe.add_(1.0)
        rc = _raw(eng, x, k_sq, rhs, 1, batch, restart, 0.0, 2, 1.0, basis, zbasis, hess, rmse, k_used)
        msg = eng.lib.hn_last_error(eng.ctx).decode()
        rc0 = _raw(eng, x, k_sq, rhs, 1, batch, restart, 0.0, 0, 1.0, basis, zbasis, hess, rmse, k_used)
        rcr = _raw_refine(eng, x64, k_sq, rhs, 1, batch, restart, 1e-10, 1e-6, 2, 1.0, basis, zbasis, hess, rmse, k_used, rmse64)
    assert rc == -2 and "captur" in msg and rc0 == -2 and rcr == -2
    g.replay()                                     # the capture is still valid, and holds nothing of the library's
    torch.cuda.synchronize()
    assert probe.tolist() == [1.0] * 4
    _left_alone(bufs + (rmse64,))
    assert _raw(eng, x, k_sq, rhs, 1, batch, restart, 0.0, 2, 1.0, basis, zbasis, hess, rmse, k_used) == 0      # eager: builds the workspaces
    torch.cuda.synchronize()
    assert k_used.tolist() == [restart] * batch and bool(torch.isfinite(zbasis).all())
    eng.check_async_errors()


# ---------------------------------------------------------------------------------------------- 7
def test_preconditioned_refinement_at_96():
    """gmres64 with and without the learned preconditioner at 96^2, source [82, 48], two ring phantoms, restart 20, tol 1e-10.
    (a) a condition: the true float64 RMSE never rises by more than a factor 1 + 1e-3 from one cycle to the next (d = 0 is in the search space of the
        inner minimisation; its fp32 estimate is good to about 1e-6 of the scaled right-hand side);
    (b) the wavefield agrees with the unpreconditioned solve's within 4 x what two unpreconditioned solves (restart 20 and 30) differ by;
    (c) it converges in no more cycles than the unpreconditioned solve at the same restart (its max_cycles is that count)."""
    from helmnet_amd import IterativeSolver
    from helmnet_amd.phantoms import ring_sos_batch
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(DEV)
    s.set_domain_size(96, source_location=[82, 48])
    sos = torch.from_numpy(ring_sos_batch(96, 2, seed=11)).to(DEV)
    tol, restart = 1e-10, 20
    plain = s.gmres64(sos, restart=restart, max_cycles=4000, tol=tol)
    other = s.gmres64(sos, restart=30, max_cycles=4000, tol=tol)
    assert plain["converged"] and other["converged"]
    pre = s.gmres64(sos, restart=restart, max_cycles=plain["cycles"], tol=tol, precondition="learned")
    print(f"cycles: unpreconditioned {plain['cycles']} (restart 30: {other['cycles']}), preconditioned {pre['cycles']}; unet evaluations "
          f"{plain['unet_evaluations']} / {pre['unet_evaluations']}; final rmse64 {plain['residual_norm64'].tolist()} / {pre['residual_norm64'].tolist()}")
    hist = torch.stack(pre["residual_norms"]).cpu().numpy()
    rise = float((hist[1:] / hist[:-1]).max()) if hist.shape[0] > 1 else 0.0
    print(f"(a) largest rise of the true float64 RMSE from one cycle to the next: factor {rise:.6f}, bar {1 + 1e-3}")
    assert rise <= 1.0 + 1e-3
    bar = 4.0 * float((plain["wavefield"] - other["wavefield"]).abs().max())
    diff = float((pre["wavefield"] - plain["wavefield"]).abs().max())
    print(f"(b) max |preconditioned - unpreconditioned| {diff:.3e}, bar 4 x {bar / 4:.3e}")
    assert diff <= bar
    assert plain["unet_evaluations"] == 0 and pre["unet_evaluations"] == pre["cycles"] * restart * 10
    assert pre["converged"] and pre["cycles"] <= plain["cycles"]              # (c)
    assert float(pre["residual_norm64"].max()) < tol
    s.engine().check_async_errors()
