"""Forward mode through the solver (hn_step_jvp, the jvp methods of helmnet_amd.autograd, IterativeSolver.jvp / linearize) against forward AD of the
CPU oracle in float64, teacher-forced at the GPU's own tape (tests/jvp_common.py).  Needs a real MI355X: ``python -m pytest tests -m gpu``.

Bars, per tensor (L_inf relative to the tensor's max, relative L2) -- the reverse-mode rows of DESIGN.md's tolerance table:
  * one iteration:              (1e-4, 5e-3)
  * three chained iterations:   (1e-3, 5e-3)
  * smooth activations:         4 x the oracle's own fp32-vs-float64 error on the same inputs
  * duality with hn_step_vjp:   4 x the largest figure the oracle's fp32 forward AD and fp32 autograd give for the same pairs
  * get_residual / apply_laplacian: L_inf 1e-5 (the operator bar)
Every oracle comparison carries the precondition of jvp_common.oracle_precondition (the oracle's fp32 forward AD within 1e-5 of its float64 one for the
piecewise-linear activations): a failing precondition FAILS the test.  Measured figures: DESIGN.md 4.14 and the forward-mode row of the table."""
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import jvp_common as J
from config_solver import DEV, _solver
from helmnet_amd.engine import Engine, _ptr, pack_weights
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _case_solver(c):
    s = _solver(c["depth"], c["act"], c["sd"], c["w_np"], c["n"], zero_source=False)
    s.set_source_maps(c["src"][:1].to(DEV))
    return s


def _dev(x):
    return None if x is None else x.float().to(DEV).contiguous()


def _tape(eng, c, K, src):
    """K iterations of hn_step from the case's inputs: (the start on the device, the three histories, k_sq)."""
    n, b = c["n"], c["b"]
    start = tuple(_dev(c[k]) for k in ("wf", "res", "st"))
    k_sq = _dev(c["k_sq"])
    wf, res, st = (t.clone() for t in start)
    wh, rh, sh = (torch.empty(K, b, 2, n, n, device=DEV), torch.empty(K, b, 2, n, n, device=DEV), torch.empty(K, b, 2, eng.state_len, device=DEV))
    eng.step(wf, res, st, k_sq, src, K, rh, wh, sh)
    return start, (wh, rh, sh), k_sq


def _jvp(eng, start, tape, k_sq, src_batch, tan, hist=True):
    """hn_step_jvp over ``tape`` along ``tan`` (CPU or device tensors; a missing key = NULL): the final tangents and the three tangent histories."""
    t = {k: _dev(tan[k]).clone() if tan.get(k) is not None else torch.zeros_like(like) for k, like in zip(("wf", "res", "st"), start)}
    h = [torch.empty_like(x) for x in tape] if hist else [None] * 3
    eng.step_jvp(*start, k_sq, src_batch, *tape, t["wf"], t["res"], t["st"], _dev(tan.get("k_sq")), _dev(tan.get("src")), *h)
    torch.cuda.synchronize()
    return t, dict(zip(("wf", "res", "st"), h))


def _compare(label, got, want, bar):
    e = {k: J.errs(got[k], want[k]) for k in want}
    print(f"[{label}] " + ", ".join(f"{k} L_inf {v[0]:.2e} L2 {v[1]:.2e}" for k, v in e.items()))
    bars = bar if isinstance(bar, dict) else {k: bar for k in e}
    bad = {k: (v, bars[k]) for k, v in e.items() if not (v[0] <= bars[k][0] and v[1] <= bars[k][1])}
    assert not bad, f"{label}: above the bar: {bad}\nall: {e}"
    return e


def _against_oracle(c, K, src_batch, bar, label, tan=None):
    s = _case_solver(c)
    eng = s.engine()
    src = _dev(c["src"])
    start, tape, k_sq = _tape(eng, c, K, src)
    tan = c["tan"] if tan is None else tan
    last, hist = _jvp(eng, start, tape, k_sq, src_batch, tan)
    cpu_tape = tuple(h.cpu() for h in tape)
    want, own = J.oracle_precondition(c, cpu_tape, tan, K)
    print(f"[{label}] oracle fp32 vs float64: " + ", ".join(f"{k} L_inf {v[0]:.2e} L2 {v[1]:.2e}" for k, v in own.items()))
    if bar == "oracle":   # the smooth activations: 4 x the fp32 oracle's own distance from float64, per tensor and measure
        bar = {k: (4 * v[0], 4 * v[1]) for k, v in own.items()}
    e = _compare(label, hist, want, bar)
    for k in hist:   # the in / out tensors hold the last slot
        assert torch.equal(last[k], hist[k][-1]), k
    return e, own


# ---- 1. one iteration, every input tangent at once ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,src_batch", [(16, 1), (16, 2), (80, 1), (80, 2)])
def test_one_iteration_every_input_tangent(n, src_batch):
    """n = 16: levels 16 .. 2 and a 1 x 1 bottleneck, every tile larger than the image.  n = 80: 80 .. 10 and a 5 x 5 bottleneck, ragged tiles, the
    prime-factor spectral route."""
    c = J.make_case(n, 2, 1, src_batch=src_batch)
    _against_oracle(c, 1, src_batch, (1e-4, 5e-3), f"one iteration n={n} src_batch={src_batch}")


# ---- 2. three chained iterations with all three tangent histories -------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(32, 1), (80, 2)])
def test_three_chained_iterations(n, seed):
    c = J.make_case(n, 2, seed)
    _against_oracle(c, 3, 1, (1e-3, 5e-3), f"three iterations n={n} seed={seed}")


# ---- 3. every route of the network, one iteration ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", J.KINKED + J.SMOOTH)
def test_every_activation(act):
    c = J.make_case(32, 2, 1, act=act)
    _against_oracle(c, 1, 1, (1e-4, 5e-3) if act in J.KINKED else "oracle", f"activation {act}")


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 6])
def test_every_depth(depth):
    c = J.make_case(64, 2, 700 + depth, depth=depth)   # depth 6: a 1 x 1 bottleneck
    _against_oracle(c, 1, 1, (1e-4, 5e-3), f"depth {depth}")


def test_state_depth_2_passes_the_stateless_slots_through():
    """Depth 4 with state_depth 2 on the autograd path the solver takes (Solve, with the solver's own list of stateless slots): the levels without state
    hand their slot -- and its tangent -- through unchanged; everything else against the oracle, which does the same."""
    from helmnet_amd.autograd import Solve, SolveSpec
    n, b, K = 32, 2, 2
    c = J.make_case(n, b, 1, sd=2)
    s = _case_solver(c)
    eng = s.engine()
    stateless = [tuple(bd) for d, bd in enumerate(s.f.state_boundaries) if d >= s.f.state_depth]
    assert stateless == [(32 * 32 + 16 * 16, 32 * 32 + 16 * 16 + 64), (32 * 32 + 16 * 16 + 64, c["L"])]
    blob = torch.from_numpy(pack_weights(c["w"], 4, "prelu", 2)).to(DEV)
    spec = SolveSpec(eng, K, 1, True, True, True, stateless)
    tan = c["tan"]
    with fwAD.dual_level():
        duals = [fwAD.make_dual(_dev(c[k]), _dev(tan[k])) for k in ("wf", "res", "st", "k_sq", "src")]
        outs = Solve.apply(spec, *duals, blob)
        prim = [fwAD.unpack_dual(o).primal.detach().cpu() for o in outs[:3]]
        got = dict(zip(("wf", "res", "st"), (fwAD.unpack_dual(o).tangent.detach().clone() for o in outs[:3])))
    a0 = stateless[0][0]
    for i in range(K):
        assert torch.equal(got["st"][i][:, :, a0:].cpu(), tan["st"][:, :, a0:]) and torch.equal(prim[2][i][:, :, a0:], c["st"][:, :, a0:])
    want, _ = J.oracle_precondition(c, tuple(prim), tan, K)
    _compare("state_depth 2", got, want, (1e-3, 5e-3))


# ---- 4. duality with the reverse mode ---------------------------------------------------------------------------------------------------
def test_duality_with_step_vjp():
    """<g, J t> against <J^T g, t> for three random (g, t): J t from hn_step_jvp, J^T g from hn_step_vjp without weight gradients, both linearised at the
    same tape; inner products in float64.  The bar: 4 x the largest figure of the oracle's fp32 forward AD against its fp32 autograd."""
    n, b, K = 32, 2, 3
    c = J.make_case(n, b, 1)
    s = _case_solver(c)
    eng = s.engine()
    src = _dev(c["src"])
    start, tape, k_sq = _tape(eng, c, K, src)
    blob = torch.from_numpy(pack_weights(c["w"], 4, "prelu", 4)).to(DEV)
    dot = lambda x, y: float((x.double().cpu() * y.double().cpu()).sum())  # noqa: E731
    norm = lambda xs: float(sum(x.double().pow(2).sum() for x in xs) ** 0.5)  # noqa: E731
    keys = ("wf", "res", "st")
    gpu, cpu = [], []
    for pair in range(3):
        g = torch.Generator().manual_seed(40 + pair)
        rnd = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
        t = {"wf": rnd(b, 2, n, n), "res": 5e-3 * rnd(b, 2, n, n), "st": 0.5 * rnd(b, 2, c["L"]), "k_sq": 0.1 * rnd(b, 1, n, n), "src": rnd(1, 2, n, n)}
        cot = {"wf": rnd(K, b, 2, n, n), "res": rnd(K, b, 2, n, n), "st": rnd(K, b, 2, c["L"])}
        _, jt = _jvp(eng, start, tape, k_sq, 1, t)
        g_k, g_s = torch.zeros_like(k_sq), torch.zeros(1, 2, n, n, device=DEV)
        o = eng.step_vjp(blob, *start, k_sq, 1, *tape, _dev(cot["wf"]), _dev(cot["res"]), _dev(cot["st"]), g_k_sq=g_k, g_src=g_s)
        torch.cuda.synchronize()
        jtg = {"wf": o["grad_wf"], "res": o["grad_res"], "st": o["grad_states"], "k_sq": g_k, "src": g_s}
        lhs, rhs = sum(dot(cot[k], jt[k]) for k in keys), sum(dot(jtg[k], t[k]) for k in t)
        gpu.append(abs(lhs - rhs) / (norm(cot.values()) * norm(jt[k].cpu() for k in keys)))
        # the oracle in fp32, both modes on one free-running fp32 trajectory from the same inputs
        f_jt = J.oracle_jvp(c, None, t, K, torch.float32)
        tab = O.SpectralTables(n, 8, 2, 1.0, dtype=torch.float32)
        leaves = {k: c[k].clone().requires_grad_(True) for k in ("wf", "res", "st", "k_sq", "src")}
        a, r, h = leaves["wf"], leaves["res"], O.unflatten_states(leaves["st"], n, 4)
        loss = 0
        for i in range(K):
            a, r, h = O.single_step(a, leaves["k_sq"], r, h, c["w"], leaves["src"], tab)
            loss = loss + (cot["wf"][i] * a).sum() + (cot["res"][i] * r).sum() + (cot["st"][i] * O.flatten_states(h)).sum()
        loss.backward()
        lhs, rhs = sum(dot(cot[k], f_jt[k]) for k in keys), sum(dot(leaves[k].grad, t[k]) for k in t)
        cpu.append(abs(lhs - rhs) / (norm(cot.values()) * norm(f_jt[k] for k in keys)))
    print(f"[duality] hn_step_jvp vs hn_step_vjp: {['%.2e' % v for v in gpu]}; oracle fp32 forward AD vs fp32 autograd: {['%.2e' % v for v in cpu]}")
    assert all(v <= 4 * max(cpu) for v in gpu), (gpu, cpu)


# ---- 5. exact properties ------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_exact_properties():
    n, b, K = 32, 3, 4
    c = J.make_case(n, b, 1)
    s = _case_solver(c)
    eng = s.engine()
    src = _dev(c["src"])
    start, tape, k_sq = _tape(eng, c, K, src)
    tan = c["tan"]
    last, hist = _jvp(eng, start, tape, k_sq, 1, tan)
    # all-zero tangents (NULL directions, and explicit zeros) give all-zero outputs
    for z in ({}, {k: torch.zeros_like(v) for k, v in tan.items()}):
        l0, h0 = _jvp(eng, start, tape, k_sq, 1, z)
        assert all(not v.any() for v in l0.values()) and all(not v.any() for v in h0.values())
    # J(2 t) == 2 J(t), two calls give equal bits
    l2, h2 = _jvp(eng, start, tape, k_sq, 1, {k: 2 * v for k, v in tan.items()})
    assert all(torch.equal(h2[k], 2 * hist[k]) for k in hist) and all(torch.equal(l2[k], 2 * last[k]) for k in last)
    again_l, again_h = _jvp(eng, start, tape, k_sq, 1, tan)
    assert _same(again_l, last) and _same(again_h, hist)
    # one call equals 2 + 2: the second fed the first's tangents and the tape's slot 1 as its start
    la, ha = _jvp(eng, start, tuple(h[:2] for h in tape), k_sq, 1, tan)
    lb, hb = _jvp(eng, tuple(h[1] for h in tape), tuple(h[2:] for h in tape), k_sq, 1, {**tan, **la})
    assert _same(lb, last) and all(torch.equal(torch.cat([ha[k], hb[k]]), hist[k]) for k in hist)
    # sample 1 of the batch of 3 equals that sample alone
    one = lambda x: x[1:2].contiguous()  # noqa: E731
    l1, h1 = _jvp(eng, tuple(one(x) for x in start), tuple(h[:, 1:2].contiguous() for h in tape), one(k_sq), 1,
                  {k: (one(v) if k != "src" else v) for k, v in tan.items()})
    assert all(torch.equal(h1[k], hist[k][:, 1:2]) for k in hist) and all(torch.equal(l1[k], last[k][1:2]) for k in last)
    # t_res of every iteration is hn_residual(t_wf, k_sq, s~), s~ = src' - k_sq' * wf_t composed here: one rounded product, one rounded difference
    t_k, t_s = _dev(tan["k_sq"]), _dev(tan["src"])
    for i in range(K):
        s_tilde = (t_s - t_k * tape[0][i]).contiguous()
        assert torch.equal(eng.residual(hist["wf"][i].contiguous(), k_sq, s_tilde), hist["res"][i]), i
    # without directions on k_sq and the source: the zero-source form
    l0, h0 = _jvp(eng, start, tape, k_sq, 1, {k: tan[k] for k in ("wf", "res", "st")})
    zero = torch.zeros(1, 2, n, n, device=DEV)
    assert all(torch.equal(eng.residual(h0["wf"][i].contiguous(), k_sq, zero), h0["res"][i]) for i in range(K))
    # every tensor one float past a 16-byte boundary: the same bits
    def off(x):
        buf = torch.empty(x.numel() + 1, device=DEV)
        v = buf[1:].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4
        return v
    t_off = {k: off(_dev(v)) for k, v in tan.items()}
    h_off = [off(torch.zeros_like(x)) for x in tape]
    eng.step_jvp(*(off(x) for x in start), off(k_sq), 1, *(off(x) for x in tape), t_off["wf"], t_off["res"], t_off["st"], t_off["k_sq"], t_off["src"], *h_off)
    torch.cuda.synchronize()
    assert all(torch.equal(a, hist[k]) for a, k in zip(h_off, ("wf", "res", "st"))) and all(torch.equal(t_off[k], last[k]) for k in last)


# ---- 6. refusals, each with every output buffer untouched -------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    n, b, K = 32, 2, 2
    c = J.make_case(n, b, 1)
    s = _case_solver(c)
    eng = s.engine()
    lib = eng.lib
    src = _dev(c["src"])
    start, tape, k_sq = _tape(eng, c, K, src)
    big = torch.full((2 * K * b * 2 * n * n,), -7.0, device=DEV)   # room for overlapping views
    fill = lambda like: torch.full_like(like, -7.0)  # noqa: E731
    t = [fill(x) for x in start]
    th = [fill(x) for x in tape]
    t_k, t_s = _dev(c["tan"]["k_sq"]), _dev(c["tan"]["src"])

    def call(ctx=None, **kw):
        a = dict(wf0=start[0], res0=start[1], states0=start[2], k_sq=k_sq, wf_hist=tape[0], res_hist=tape[1], st_hist=tape[2], t_wf=t[0], t_res=t[1],
                 t_states=t[2], t_k_sq=t_k, t_src=t_s, t_wf_hist=th[0], t_res_hist=th[1], t_st_hist=th[2], src_batch=1, batch=b, n_iter=K)
        a.update(kw)
        p = lambda k: _ptr(a[k])  # noqa: E731
        return lib.hn_step_jvp(ctx or eng.ctx, p("wf0"), p("res0"), p("states0"), p("k_sq"), a["src_batch"], a["batch"], a["n_iter"], p("wf_hist"),
                               p("res_hist"), p("st_hist"), p("t_wf"), p("t_res"), p("t_states"), p("t_k_sq"), p("t_src"), p("t_wf_hist"), p("t_res_hist"),
                               p("t_st_hist"), eng._stream())

    def untouched():
        torch.cuda.synchronize()
        return all(bool((x == -7.0).all()) for x in t + th + [big])

    err = lambda: lib.hn_last_error(eng.ctx).decode()  # noqa: E731
    for name in ("wf0", "res0", "states0", "k_sq", "wf_hist", "res_hist", "st_hist", "t_wf", "t_res", "t_states"):
        assert call(**{name: None}) == -1 and untouched(), name
    assert call(n_iter=0) == -1 and call(batch=0) == -1 and call(src_batch=3) == -1 and untouched()
    # a written tensor may overlap nothing: t_wf inside wf_hist, t_wf_hist over t_wf
    assert call(t_wf=tape[0][1]) == -1 and "wf_hist overlaps t_wf" in err() and untouched()
    view = big[: b * 2 * n * n].view(b, 2, n, n)
    assert call(t_wf=view, t_wf_hist=big[4: 4 + K * b * 2 * n * n].view(K, b, 2, n, n)) == -1 and "t_wf overlaps t_wf_hist" in err() and untouched()
    # tensors that are only read may share memory
    assert call(res0=start[0], t_src=None, t_k_sq=None, n_iter=1, wf_hist=tape[0][:1], res_hist=tape[0][:1], st_hist=tape[2][:1], t_wf_hist=None,
                t_res_hist=None, t_st_hist=None, t_wf=torch.zeros_like(start[0]), t_res=torch.zeros_like(start[0]), t_states=torch.zeros_like(start[2])) == 0
    assert untouched()
    eng.set_unet_precision("fp16")
    try:
        assert call() == -3 and untouched()
    finally:
        eng.set_unet_precision("fp32")
    fresh = Engine(torch.device(DEV))
    try:
        assert call(ctx=fresh.ctx) == -2
        fresh.set_domain(n, 8, 2.0, 1.0)
        assert call(ctx=fresh.ctx) == -2 and untouched()     # still no weights
    finally:
        fresh.close()


def test_first_call_under_capture_is_refused_and_the_second_replays_to_the_eager_bits():
    n, b, K = 32, 2, 2
    c = J.make_case(n, b, 1)
    s = _case_solver(c)
    eng = s.engine()
    start, tape, k_sq = _tape(eng, c, K, _dev(c["src"]))
    key = eng.domain_key
    eng.set_domain(16, *key[1:])
    eng.set_domain(*key)               # a fresh domain: no forward-mode workspace yet
    tan = {k: _dev(v) for k, v in c["tan"].items()}
    t = [torch.full_like(x, -7.0) for x in start]

    def call():
        return eng.lib.hn_step_jvp(eng.ctx, *(_ptr(x) for x in start), _ptr(k_sq), 1, b, K, *(_ptr(x) for x in tape), *(_ptr(x) for x in t), _ptr(tan["k_sq"]),
                                   _ptr(tan["src"]), None, None, None, eng._stream())

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = call()
        assert rc == -2 and "capture" in eng.lib.hn_last_error(eng.ctx).decode()
        torch.cuda.synchronize()
        assert all(bool((x == -7.0).all()) for x in t)
        want, _ = _jvp(eng, start, tape, k_sq, 1, c["tan"], hist=False)     # eager: builds the workspace
        for x, k in zip(t, ("wf", "res", "st")):
            x.copy_(tan[k])
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = call()
        assert rc == 0
        graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(x, want[k]) for x, k in zip(t, ("wf", "res", "st")))


# ---- 7. the Python surface -----------------------------------------------------------------------------------------------------------------
def _py_solver(n):
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights().to(DEV)
    s.freeze()
    s.set_domain_size(n, source_location=[n // 3, n // 2])
    return s


def test_forward_ad_through_forward_equals_step_jvp_on_the_same_tape():
    from helmnet_amd.phantoms import ring_sos_batch
    from helmnet_amd.solver import jvp_initial_tangents
    n, b, K = 32, 2, 6
    s = _py_solver(n).differentiable()
    eng = s.engine()
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=5)).to(DEV)
    d_sos = 0.1 * torch.randn(b, 1, n, n, generator=torch.Generator().manual_seed(1)).to(DEV)
    runs = []
    for ck in (1, 4):
        with fwAD.dual_level():
            out = s.forward(fwAD.make_dual(sos, d_sos), num_iterations=K, return_wavefields=True, return_states=True, checkpoint_every=ck)
            wf = [fwAD.unpack_dual(x) for x in out["wavefields"]]
            res = [fwAD.unpack_dual(x) for x in out["residuals"]]
            st = [fwAD.unpack_dual(x) for x in out["states"]]
            rm = fwAD.unpack_dual(out["residual_norms"])
            runs.append(dict(tape=tuple(torch.stack([x.primal.detach() for x in h]) for h in (wf, res, st)),
                             tan=tuple(torch.stack([x.tangent.detach().clone() for x in h]) for h in (wf, res, st)),
                             rmse=rm.primal.detach().clone(), t_rmse=rm.tangent.detach().clone()))
    r = runs[0]
    for k in ("tape", "tan"):
        assert all(torch.equal(x, y) for x, y in zip(runs[1][k], r[k])), k     # checkpoint_every = 4: the same bits
    assert torch.equal(runs[1]["t_rmse"], r["t_rmse"])
    with fwAD.dual_level():   # nothing but the last wavefield and the norms kept: the residual tangents live one segment at a time
        out = s.forward(fwAD.make_dual(sos, d_sos), num_iterations=K, checkpoint_every=4, residuals="norms")
        assert len(out["wavefields"]) == 1
        assert torch.equal(fwAD.unpack_dual(out["wavefields"][-1]).tangent, r["tan"][0][-1])
        assert torch.equal(fwAD.unpack_dual(out["residual_norms"]).tangent, r["t_rmse"])
    k_sq = ((float(s.hparams.omega) / sos) ** 2).contiguous()
    src = s._src()
    wf0 = torch.zeros(b, 2, n, n, device=DEV)
    res0 = eng.residual(wf0, k_sq, src)
    st0 = torch.zeros(b, 2, eng.state_len, device=DEV)
    _, t_wf, t_res = jvp_initial_tangents(float(s.hparams.omega), sos, d_sos, None)
    with fwAD.dual_level():   # k_sq' as torch's own rules round it on the way through get_initials (the closed form differs in the last bit)
        t_k = fwAD.unpack_dual(s.get_initials(fwAD.make_dual(sos, d_sos))[0]).tangent.clone().contiguous()
    t_st = torch.zeros_like(st0)
    th = [torch.empty_like(x) for x in r["tape"]]
    eng.step_jvp(wf0, res0, st0, k_sq, 1, *r["tape"], t_wf, t_res, t_st, t_k, None, *th)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(th, r["tan"]))
    want_rmse = (r["tape"][1] * th[1]).sum((-3, -2, -1)) / (2 * n * n * r["rmse"])
    assert torch.equal(r["t_rmse"], want_rmse)
    # a tangent on the weight blob raises
    from helmnet_amd.autograd import Solve, SolveSpec, weight_blob
    blob = weight_blob(s.f).detach()
    with fwAD.dual_level():
        with pytest.raises(NotImplementedError, match="weight"):
            Solve.apply(SolveSpec(eng, 1, 1, False, False, False, []), wf0, res0, st0, k_sq, src, fwAD.make_dual(blob, torch.ones_like(blob)))


def test_solver_jvp_chunks_equal_linearize():
    from helmnet_amd.phantoms import ring_sos_batch
    n, b, K = 32, 2, 6
    s = _py_solver(n)
    sos = torch.from_numpy(ring_sos_batch(n, b, seed=5)).to(DEV)
    g = torch.Generator().manual_seed(2)
    d_sos, d_src = 0.1 * torch.randn(b, 1, n, n, generator=g).to(DEV), torch.randn(1, 2, n, n, generator=g).to(DEV)
    a = s.jvp(sos, d_sos, d_src, num_iterations=K, chunk=4)
    c = s.jvp(sos, d_sos, d_src, num_iterations=K, chunk=6)
    lin = s.linearize(sos, num_iterations=K)
    l1, l2 = lin.jvp(d_sos, d_src), lin.jvp(d_sos=d_sos)
    assert torch.equal(a["wavefield"], lin.wavefield) and torch.equal(a["residual"], lin.residual) and torch.equal(c["wavefield"], lin.wavefield)
    for k in ("d_wavefield", "d_residual", "d_rmse"):
        assert torch.equal(a[k], l1[k]) and torch.equal(c[k], l1[k]), k
    assert float(a["d_wavefield"].abs().max()) > 0 and not torch.equal(l2["d_wavefield"], l1["d_wavefield"])
    only_sos = s.jvp(sos, d_sos, None, num_iterations=K, chunk=5)
    assert torch.equal(only_sos["d_wavefield"], l2["d_wavefield"])
    # the plain solve is what it always was
    ref = s.forward(sos, num_iterations=K)
    assert torch.equal(ref["wavefields"][-1], a["wavefield"])


def test_forward_ad_through_the_operators_against_float64():
    n, b = 32, 2
    s = _py_solver(n).differentiable()
    g = torch.Generator().manual_seed(3)
    rnd = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
    wf, t_wf, k_sq, t_k = rnd(b, 2, n, n), rnd(b, 2, n, n), 0.25 + torch.rand(b, 1, n, n, generator=g), 0.1 * rnd(b, 1, n, n)
    with fwAD.dual_level():
        x = fwAD.make_dual(wf.to(DEV), t_wf.to(DEV))
        got_res = fwAD.unpack_dual(s.get_residual(x, fwAD.make_dual(k_sq.to(DEV), t_k.to(DEV)))).tangent.clone()
        got_lap = fwAD.unpack_dual(s.apply_laplacian(x)).tangent.clone()
    tab = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
    src = s.source.detach().cpu().to(F64)
    with fwAD.dual_level():
        x = fwAD.make_dual(wf.to(F64), t_wf.to(F64))
        want_res = fwAD.unpack_dual(O.get_residual(x, fwAD.make_dual(k_sq.to(F64), t_k.to(F64)), src, tab)).tangent.clone()
        want_lap = fwAD.unpack_dual(O.apply_laplacian(x, tab)).tangent.clone()
    e = {"get_residual": J.errs(got_res, want_res)[0], "apply_laplacian": J.errs(got_lap, want_lap)[0]}
    print(f"[operators] L_inf {e}")
    assert all(v <= 1e-5 for v in e.values()), e
