"""Reverse mode through the solver (hn_step_vjp, helmnet_amd.autograd) against float64 autograd of the CPU oracle.
Needs a real MI355X: ``python -m pytest tests -m gpu``.

Bars (DESIGN.md tolerance table, reverse-mode rows), per tensor relative L2 <= 5e-3 and L_inf relative to the tensor's max:
  * one iteration:                     1e-4 (the training bar of one unrolled iteration)
  * a few chained iterations (<= 3):   1e-3 (the bar of the training step's unrolled iterations: the iteration amplifies rounding)
  * 20 iterations from the sound speed, against the free-running float64 solve: relative L2 only (the fp32 trajectory drifts from the
    float64 one, and the gradients are taken along it); against the float64 reverse sweep linearised at the solve's own stored
    trajectory (teacher-forced, the drift drops out): L_inf 1e-3 and relative L2 1e-3 for sos and every weight tensor
  * against the REFERENCE's autograd (tests/golden/vjp.npz, make_golden_vjp.py): relative L2 <= 5e-3
"""
import numpy as np
import pytest
import torch

from config_weights import config_weights
from golden_inputs import teacher_inputs
from helmnet_amd.engine import pack_weights
from helmnet_amd.phantoms import ring_sos_batch
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def _errs(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    linf = float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))
    l2 = float((got - want).norm() / want.norm().clamp_min(1e-30))
    return linf, l2


def _check(pairs, linf_bar=1e-4, l2_bar=5e-3):
    errs = {k: _errs(g, w) for k, (g, w) in pairs.items()}
    bad = {k: v for k, v in errs.items() if not (v[0] <= linf_bar and v[1] <= l2_bar)}
    assert not bad, f"above ({linf_bar}, {l2_bar}): {bad}\nall: {errs}"


def _solver():
    from helmnet_amd import IterativeSolver
    return IterativeSolver.from_exported_weights().to(DEV)


def _fweights(solver):
    return {k: v.detach().cpu() for k, v in solver.f.state_dict().items()}


def _oracle_vjp(w, wf, res, st, k_sq, src, n, K, cot, depth=4, act="prelu", state_depth=None):
    """float64 oracle: K iterations from (wf, res, st); loss = sum of <cot, output> over the histories; returns input and weight grads."""
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
    w64 = {k: v.to(F64).requires_grad_(True) for k, v in w.items()}
    wf, res, st, k_sq, src = (x.to(F64).requires_grad_(True) for x in (wf, res, st, k_sq, src))
    states = O.unflatten_states(st, n, depth)
    a, b_, c = wf, res, states
    loss = 0
    for i in range(K):
        a, b_, c = O.single_step(a, k_sq, b_, c, w64, src, t, depth, act, state_depth=state_depth)
        loss = loss + (cot["wf"][i].to(F64) * a).sum() + (cot["res"][i].to(F64) * b_).sum() + (cot["st"][i].to(F64) * O.flatten_states(c)).sum()
    loss.backward()
    return {"wf": wf.grad, "res": res.grad, "st": st.grad, "k_sq": k_sq.grad, "src": src.grad}, {k: v.grad for k, v in w64.items()}


def _cot(K, b, n, L, seed):
    g = torch.Generator().manual_seed(seed)
    return {"wf": torch.randn(K, b, 2, n, n, generator=g), "res": 1e3 * torch.randn(K, b, 2, n, n, generator=g),
            "st": torch.randn(K, b, 2, L, generator=g)}


def _engine_vjp(solver, w, ti, K, cot, src_batch=1):
    eng = solver.engine()
    n, b = eng.n, ti["wf"].shape[0]
    d = lambda x: torch.as_tensor(x).float().to(DEV).contiguous()  # noqa: E731
    blob = d(pack_weights(w, solver.f.depth, solver.f.activation_function, solver.f.state_depth))
    wf0, res0, st0, k_sq = d(ti["wf"]), d(ti["res"]), d(ti["states"]), d(1.0 / ti["sos"] ** 2)
    src = d(solver.source.detach()) if src_batch == 1 else d(torch.randn(b, 2, n, n))
    wf, res, st = wf0.clone(), res0.clone(), st0.clone()
    wh, rh, sh = (torch.empty(K, b, 2, n, n, device=DEV), torch.empty(K, b, 2, n, n, device=DEV), torch.empty(K, b, 2, eng.state_len, device=DEV))
    eng.step(wf, res, st, k_sq, src, K, rh, wh, sh)
    g_k, g_s, g_w = torch.zeros_like(k_sq), torch.zeros(src_batch, 2, n, n, device=DEV), torch.zeros_like(blob)
    out = eng.step_vjp(blob, wf0, res0, st0, k_sq, src_batch, wh, rh, sh, d(cot["wf"]), d(cot["res"]), d(cot["st"]), g_k_sq=g_k, g_src=g_s, g_weights=g_w)
    torch.cuda.synchronize()
    return out, g_k, g_s, g_w, src


def _weight_pairs(g_w, w_grads, depth):
    from helmnet_amd.engine import weight_shapes
    pairs, pos = {}, 0
    for name, shape in weight_shapes(depth).items():
        m = int(np.prod(shape))
        if name in w_grads and w_grads[name] is not None:
            pairs["w:" + name] = (g_w[pos:pos + m].reshape(shape), w_grads[name])
        pos += m
    return pairs


@pytest.mark.parametrize("n,b", [(96, 2), (128, 1)])
def test_one_iteration_every_input_gradient(n, b):
    solver = _solver()
    solver.set_domain_size(n, source_location=[n // 3, n // 2])
    w = _fweights(solver)
    ti = teacher_inputs(n, b, seed=300 + n)
    L = solver.engine().state_len
    cot = _cot(1, b, n, L, seed=n)
    out, g_k, g_s, g_w, src = _engine_vjp(solver, w, ti, 1, cot)
    want, wg = _oracle_vjp(w, torch.from_numpy(ti["wf"]), torch.from_numpy(ti["res"]), torch.from_numpy(ti["states"]),
                           torch.from_numpy(1.0 / ti["sos"] ** 2), src.cpu(), n, 1, cot)
    pairs = {"wf0": (out["grad_wf"], want["wf"]), "res0": (out["grad_res"], want["res"]), "st0": (out["grad_states"], want["st"]),
             "k_sq": (g_k, want["k_sq"]), "src": (g_s, want["src"])}
    pairs.update(_weight_pairs(g_w.cpu(), wg, 4))
    _check(pairs)


def test_k20_through_forward_sos_and_weights():
    n, b, K = 96, 3, 20
    solver = _solver()
    solver.set_domain_size(n, source_location=[30, 48])
    w = _fweights(solver)
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=5))
    cot = _cot(K, b, n, solver.engine().state_len, seed=7)
    sos_d = sos.to(DEV).requires_grad_(True)
    out = solver.forward(sos_d, num_iterations=K, return_wavefields=True, return_states=True, residuals="all")
    loss = sum((cot["wf"][i].to(DEV) * out["wavefields"][i]).sum() + (1e-3 * cot["res"][i].to(DEV) * out["residuals"][i]).sum()
               for i in range(K))
    loss.backward()

    def oracle(dtype):
        t = O.SpectralTables(n, 8, 2, 1.0, dtype=dtype)
        wd = {k: v.to(dtype).requires_grad_(True) for k, v in w.items()}
        sd = sos.to(dtype).requires_grad_(True)
        src = solver.source.detach().cpu().to(dtype)
        k_sq, wf = O.get_initials(sd, 1.0)
        states = [torch.zeros(b, 2, m, m, dtype=dtype) for m in O.state_dims(n, 4)]
        res = O.get_residual(wf, k_sq, src, t)
        lo = 0
        for i in range(K):
            wf, res, states = O.single_step(wf, k_sq, res, states, wd, src, t)
            lo = lo + (cot["wf"][i].to(dtype) * wf).sum() + (1e-3 * cot["res"][i].to(dtype) * res).sum()
        lo.backward()
        return {"sos": sd.grad, **{k: v.grad for k, v in wd.items()}}

    # (a) the free-running float64 solve: the fp32 trajectory drifts from it over 20 iterations, so relative L2 only
    want = oracle(F64)
    params = dict(solver.f.named_parameters())
    got = {"sos": sos_d.grad, **{k: p.grad for k, p in params.items()}}
    some = ("sos", "inc.double_conv.0.weight", "enc.0.conv_signal.double_conv.2.weight", "enc.3.down.weight", "decode.0.double_conv.0.bias",
            "up.1.weight", "outc.conv.weight", "enc.2.conv_state.double_conv.0.weight")
    _check({k: (got[k], want[k]) for k in some}, linf_bar=float("inf"))
    # (b) teacher-forced: the float64 reverse sweep linearised at THIS solve's stored trajectory (what hn_step_vjp linearises at), so the
    # drift drops out and what is left is the kernels' arithmetic -- every weight tensor, the PReLU slopes included
    wh = torch.stack([x.detach().cpu() for x in out["wavefields"]]).to(F64)
    rh = torch.stack([x.detach().cpu() for x in out["residuals"]]).to(F64)
    sh = torch.stack([x.detach().cpu() for x in out["states"]]).to(F64)
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
    wd = {k: v.to(F64).requires_grad_(True) for k, v in w.items()}
    src = solver.source.detach().cpu().to(F64)
    k_sq = ((1.0 / sos.to(F64)) ** 2).requires_grad_(True)
    wf0 = torch.zeros(b, 2, n, n, dtype=F64)
    res0 = O.get_residual(wf0, k_sq.detach(), src, t)
    st0 = torch.zeros(b, 2, sh.shape[-1], dtype=F64)
    g_wf, g_res, g_st = torch.zeros_like(wf0), torch.zeros_like(wf0), torch.zeros_like(st0)
    for i in range(K - 1, -1, -1):
        a, r, h = ((wh[i - 1], rh[i - 1], sh[i - 1]) if i > 0 else (wf0, res0, st0))
        a, r, h = (x.clone().requires_grad_(True) for x in (a, r, h))
        wf, res, st = O.single_step(a, k_sq, r, O.unflatten_states(h, n, 4), wd, src, t)
        ((g_wf + cot["wf"][i].to(F64)) * wf).sum().add_(((g_res + 1e-3 * cot["res"][i].to(F64)) * res).sum()) \
            .add_((g_st * O.flatten_states(st)).sum()).backward()
        g_wf, g_res, g_st = a.grad, r.grad, h.grad
    # res0 = L(0) + k_sq * 0 - src: its cotangent reaches neither k_sq nor sos; k_sq = (1 / sos)^2
    g_sos = k_sq.grad * (-2.0 / sos.to(F64) ** 3)
    tf = {"sos": g_sos, **{k: v.grad for k, v in wd.items()}}
    errs = {k: _errs(got[k], tf[k]) for k in got}
    bad = {k: v for k, v in errs.items() if not (v[0] <= 1e-3 and v[1] <= 1e-3)}
    assert not bad, f"teacher-forced, above (1e-3, 1e-3): {bad}\nall: {errs}"


def test_checkpointing_is_bit_identical():
    n, b, K = 64, 2, 30
    solver = _solver()
    solver.set_domain_size(n, source_location=[20, 32])
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=9)).to(DEV)
    got = []
    for c in (1, 7, K):
        solver.zero_grad(set_to_none=True)
        s = sos.clone().requires_grad_(True)
        out = solver.forward(s, num_iterations=K, residuals="last", checkpoint_every=c)
        (out["wavefields"][-1][:, :, 10:50, 30].pow(2).sum() + out["residuals"][-1].pow(2).mean()).backward()
        got.append((s.grad.clone(), torch.cat([p.grad.reshape(-1) for p in solver.f.parameters()])))
    for g in got[1:]:
        assert torch.equal(g[0], got[0][0]) and torch.equal(g[1], got[0][1])


def test_reproducible_and_batch_independent():
    n, K = 64, 6
    solver = _solver()
    solver.freeze()
    solver.set_domain_size(n, source_location=[20, 32])
    sos = torch.from_numpy(ring_sos_batch(n, 4, seed=2)).to(DEV)

    def grad(x):
        x = x.clone().requires_grad_(True)
        out = solver.forward(x, num_iterations=K, residuals="last")
        scale = 2.0 ** torch.arange(x.shape[0], device=DEV)    # powers of two: exact through every rounding
        (out["wavefields"][-1].pow(2).sum(dim=(1, 2, 3)) * scale).sum().backward()
        return x.grad

    a, a2 = grad(sos), grad(sos)
    assert torch.equal(a, a2)
    one = grad(sos[2:3])
    assert torch.equal(a[2:3], 4 * one)


def test_nothing_changes_without_grad():
    n, K = 64, 5
    solver = _solver()
    solver.set_domain_size(n, source_location=[20, 32])
    sos = torch.from_numpy(ring_sos_batch(n, 2, seed=4)).to(DEV)
    ref = solver.forward(sos, num_iterations=K, return_wavefields=True)        # unfrozen, plain tensors: the plain path
    assert ref["wavefields"][-1].grad_fn is None and ref["residuals"][-1].grad_fn is None
    with torch.no_grad():
        o = solver.forward(sos.clone().requires_grad_(True), num_iterations=K)
    assert o["wavefields"][-1].grad_fn is None
    s = sos.clone().requires_grad_(True)
    g = solver.forward(s, num_iterations=K, return_wavefields=True)
    assert g["wavefields"][-1].grad_fn is not None
    for i in range(K):   # the autograd forward runs the same kernels
        assert torch.equal(g["wavefields"][i].detach(), ref["wavefields"][i])
        assert torch.equal(g["residuals"][i].detach(), ref["residuals"][i])
    solver.freeze()
    f = solver.forward(sos, num_iterations=K)
    assert f["wavefields"][-1].grad_fn is None


def test_refusals():
    solver = _solver()
    solver.set_domain_size(64, source_location=[20, 32])
    sos = torch.from_numpy(ring_sos_batch(64, 1, seed=4)).to(DEV)
    s = sos.clone().requires_grad_(True)
    out = solver.forward(s, num_iterations=2, residuals="last")
    with pytest.raises(RuntimeError):
        torch.autograd.grad(out["residuals"][-1].sum(), s, create_graph=True)
    solver.set_unet_precision("fp16")
    with pytest.raises(NotImplementedError):
        solver.forward(sos.clone().requires_grad_(True), num_iterations=2)


def test_chained_single_step_matches_n_steps_and_oracle():
    n, b = 64, 2
    solver = _solver()
    solver.freeze()
    solver.set_domain_size(n, source_location=[20, 32])
    ti = teacher_inputs(n, b, seed=21)
    k_sq = torch.from_numpy(1.0 / ti["sos"] ** 2).to(DEV)
    wf0 = torch.from_numpy(ti["wf"]).to(DEV)
    res0 = torch.from_numpy(ti["res"]).to(DEV)
    st0 = torch.from_numpy(ti["states"]).to(DEV)

    def run(chained):
        st = st0.clone().requires_grad_(True)
        wf = wf0.clone().requires_grad_(True)
        solver.f.set_states(st, flatten=True)
        if chained:
            a, r = wf, res0
            for _ in range(3):
                a, r = solver.single_step(a, k_sq, r)
        else:
            o = solver.n_steps(wf, k_sq, res0, 3, residuals="last")
            a = o["wavefields"][-1]
        hs = solver.f.get_states(flatten=True)
        (a.pow(2).sum() + hs.pow(2).sum()).backward()
        return wf.grad, st.grad

    gw_c, gs_c = run(True)
    gw_n, gs_n = run(False)
    for x, y in ((gw_c, gw_n), (gs_c, gs_n)):
        assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())
    # oracle
    w = {k: v.to(F64) for k, v in _fweights(solver).items()}
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
    wf = wf0.cpu().to(F64).requires_grad_(True)
    st = st0.cpu().to(F64).requires_grad_(True)
    a, r, h = wf, res0.cpu().to(F64), O.unflatten_states(st, n, 4)
    for _ in range(3):
        a, r, h = O.single_step(a, k_sq.cpu().to(F64), r, h, w, solver.source.detach().cpu().to(F64), t)
    (a.pow(2).sum() + O.flatten_states(h).pow(2).sum()).backward()
    _check({"wf": (gw_c, wf.grad), "st": (gs_c, st.grad)}, linf_bar=1e-3)


def test_source_gradient_and_residual_norms():
    n, b, K = 64, 2, 4
    solver = _solver()
    solver.freeze()
    solver.set_domain_size(n, source_location=[20, 32])
    solver.source.requires_grad_(True)
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=8)).to(DEV)
    out = solver.forward(sos, num_iterations=K, residuals="norms")
    out["residual_norms"].sum().backward()
    g1 = solver.source.grad.clone()
    # per-sample source maps: the sum of their gradients is the broadcast map's gradient
    solver.set_multiple_sources([[20, 32], [20, 32]])
    solver.source.requires_grad_(True)
    out = solver.forward(sos, num_iterations=K, residuals="norms")
    out["residual_norms"].sum().backward()
    g2 = solver.source.grad
    assert g2.shape[0] == b
    assert float((g2.sum(0, keepdim=True) - g1).abs().max()) <= 1e-5 * float(g1.abs().max())
    # oracle: rmse cotangent alone
    w = {k: v.to(F64) for k, v in _fweights(solver).items()}
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
    src = solver.source.detach().cpu()[:1].to(F64).requires_grad_(True)
    s64 = sos.cpu().to(F64).requires_grad_(True)
    tr = O.solve(s64, w, src, t, K)["trace"]
    torch.stack(tr).sum().backward()
    _check({"src": (g1, src.grad)})


def test_other_networks_and_stateless_slots():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.checkpoint import default_exported_weights, read_exported_weights
    n, b, K = 64, 2, 3
    for depth, act, sd in ((3, "relu", 2), (4, "gelu", 4)):
        w = config_weights(depth, seed=11, act=act, state_depth=sd, n=n)
        hp, _ = read_exported_weights(*default_exported_weights())
        hp.update(depth=depth, activation_function=act, state_depth=sd, domain_size=n)
        solver = IterativeSolver(**hp).to(DEV)
        solver.f.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in w.items()})
        solver.set_domain_size(n, source_location=[20, 32])
        ti = teacher_inputs(n, b, seed=31)
        L = sum((n >> d) ** 2 for d in range(depth))
        st0 = torch.from_numpy(ti["states"][:, :, :L].copy()).to(DEV).requires_grad_(True)
        wf0 = torch.from_numpy(ti["wf"]).to(DEV).requires_grad_(True)
        k_sq = torch.from_numpy(1.0 / ti["sos"] ** 2).to(DEV)
        solver.f.set_states(st0, flatten=True)
        o = solver.n_steps(wf0, k_sq, torch.from_numpy(ti["res"]).to(DEV), K, return_states=True, residuals="last")
        hs = o["states"][-1]
        (o["wavefields"][-1].pow(2).sum() + hs.pow(2).sum()).backward()
        # oracle
        w64 = {k: torch.as_tensor(np.asarray(v)).to(F64).requires_grad_(True) for k, v in w.items()}
        t = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
        wf = wf0.detach().cpu().to(F64).requires_grad_(True)
        st = st0.detach().cpu().to(F64).requires_grad_(True)
        a, r, h = wf, torch.from_numpy(ti["res"]).to(F64), O.unflatten_states(st, n, depth)
        for _ in range(K):
            a, r, h = O.single_step(a, k_sq.cpu().to(F64), r, h, w64, solver.source.detach().cpu().to(F64), t, depth, act, state_depth=sd)
        (a.pow(2).sum() + O.flatten_states(h).pow(2).sum()).backward()
        pairs = {"wf": (wf0.grad, wf.grad), "st": (st0.grad, st.grad)}
        params = dict(solver.f.named_parameters())
        for name, p in params.items():
            if w64.get(name) is not None and w64[name].grad is not None and float(w64[name].grad.abs().max()) > 0:
                pairs[name] = (p.grad, w64[name].grad)
        _check(pairs, linf_bar=1e-3)
        # stateless slots pass through: identity cotangent
        for d in range(sd, depth):
            a_, e_ = solver.f.state_boundaries[d]
            assert torch.allclose(st0.grad[:, :, a_:e_], 2 * st0.detach()[:, :, a_:e_], rtol=1e-6, atol=0)


def test_256_one_iteration():
    n, b = 256, 2
    solver = _solver()
    solver.set_domain_size(n, source_location=[30, 128])
    w = _fweights(solver)
    ti = teacher_inputs(n, b, seed=256)
    cot = _cot(1, b, n, solver.engine().state_len, seed=3)
    out, g_k, g_s, g_w, src = _engine_vjp(solver, w, ti, 1, cot)
    want, wg = _oracle_vjp(w, torch.from_numpy(ti["wf"]), torch.from_numpy(ti["res"]), torch.from_numpy(ti["states"]),
                           torch.from_numpy(1.0 / ti["sos"] ** 2), src.cpu(), n, 1, cot)
    pairs = {"wf0": (out["grad_wf"], want["wf"]), "res0": (out["grad_res"], want["res"]), "st0": (out["grad_states"], want["st"]),
             "k_sq": (g_k, want["k_sq"])}
    pairs.update(_weight_pairs(g_w.cpu(), wg, 4))
    _check(pairs)


def test_checkpoint_segments_on_a_fresh_workspace():
    """K = 8, c = 7: the last segment (one iteration) is processed first on a fresh context; the next segment must continue the same
    partial sums, not a re-allocated workspace.  Weights unfrozen: the weight and slope gradients are compared bit for bit."""
    n, b, K = 64, 2, 8
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=13)).to(DEV)
    got = []
    for c in (7, 1):
        solver = _solver()                      # a fresh context each time: nothing reserved yet
        solver.set_domain_size(n, source_location=[20, 32])
        s = sos.clone().requires_grad_(True)
        out = solver.forward(s, num_iterations=K, residuals="last", checkpoint_every=c)
        (out["wavefields"][-1].pow(2).sum() + out["residuals"][-1].pow(2).mean()).backward()
        got.append((s.grad.clone(), torch.cat([p.grad.reshape(-1) for p in solver.f.parameters()])))
    assert torch.equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])


def test_against_the_reference_autograd():
    """tests/golden/vjp.npz: the reference's own IterativeSolver.forward differentiated by torch (make_golden_vjp.py): 64^2 x 2, 10 iterations,
    shipped weights, the source map requiring grad; sos, source and three weight gradients within relative L2 5e-3."""
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vjp.npz")) as z:
        fix = {k: z[k] for k in z.files}
    N, LOC, ITERS, WEIGHTS = fix["sos"].shape[-1], [int(x) for x in fix["loc"]], int(fix["iters"]), [str(x) for x in fix["weight_names"]]
    solver = _solver()
    solver.set_domain_size(N, source_location=LOC)
    solver.source.requires_grad_(True)
    sos = torch.from_numpy(fix["sos"]).to(DEV).requires_grad_(True)
    out = solver.forward(sos, num_iterations=ITERS, residuals="last")
    loss = (torch.from_numpy(fix["proj"]).to(DEV) * out["wavefields"][-1]).sum() + solver.test_loss_function(out["residuals"][-1]).mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(fix["loss"])) <= 1e-4 * abs(float(fix["loss"]))
    params = dict(solver.f.named_parameters())
    pairs = {"sos": (sos.grad, torch.from_numpy(fix["grad_sos"])), "source": (solver.source.grad, torch.from_numpy(fix["grad_source"]))}
    for k in WEIGHTS:
        pairs[k] = (params[k].grad, torch.from_numpy(fix["grad_" + k]))
    _check(pairs, linf_bar=float("inf"), l2_bar=5e-3)


def test_tape_modified_in_place_raises():
    """The tape goes through save_for_backward: an output the caller changes in place makes backward raise instead of linearising around it."""
    solver = _solver()
    solver.freeze()
    solver.set_domain_size(64, source_location=[20, 32])
    s = torch.from_numpy(ring_sos_batch(64, 1, seed=4)).to(DEV).requires_grad_(True)
    out = solver.forward(s, num_iterations=3, residuals="norms")
    loss = out["residual_norms"].sum()
    out["residual_norms"].mul_(2)
    with pytest.raises(RuntimeError):
        loss.backward()
