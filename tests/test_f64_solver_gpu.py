"""The solver loop in float64 on the GPU: hn_unet_f64 / hn_step_f64, IterativeSolver.forward64 / n_steps64 / deviation_from_float64.  Needs a real MI355X.

Expected values: the oracle evaluated in float64 on the CPU (``O.unet_forward`` / ``O.single_step`` with ``.double()`` weights and float64 spectral tables:
what the reference computes after ``solver.double()``), from seeded fp32-representable inputs, once per module; and the reference's own float64
trajectory stored in tests/golden/long_run.npz.

Bars (fixed before the kernels existed; every test prints what it observed).
  UNet, 1e-12 * max|expected| per tensor: two float64 evaluations of the oracle that differ only in summation order agree to 0.9 - 1.5e-15 * max, the
  oracle in fp32 sits 4.7 - 7.0e-7 * max away: ~600 x over rounding, five orders below any fp32 contamination.
  Ten iterations, 1e-10 * max|expected|: the reference's fp32 run drifts <= 9e-4 from float64 over 1000 iterations, an amplification <= 1.5e4 of a 6e-8
  perturbation over a whole run; 1.5e4 * 1.5e-15 ~ 2e-11.
  The stored trajectory, 1e-7 * scale and 1e-6 relative on the RMSE trace: the fixture is fp32 (tests/test_long_run.py:47-67)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_inputs import long_inputs
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PML, SIGMA_MAX, K = 8, 2.0, 1.0
DEPTH = 4
BAR_UNET, BAR_STEP = 1e-12, 1e-10
ACTS = ["prelu", "relu", "leakyrelu", "celu", "tanh", "gelu", "tanhshrink", "softplus"]
# n = 16: a 1 x 1 deepest plane, 2 x 2 -> 1 x 1 stride-2 convolutions; 32 with B = 3: an odd batch of planes smaller than a tile; 48: no power of two, tile
# remainders; 96: the training size; 144: the size whose fp32 path is the dense fallback; 256: several tiles per plane at every level
UNET_CASES = [(16, 1), (32, 3), (48, 2), (96, 1), (144, 1), (256, 1)]
STEP_CASES = [(48, 2, 1), (48, 2, 2), (16, 1, 1)]
N_ITER = 10
_cache = {}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rel(got, want):
    return float((got.cpu() - want).abs().max()) / float(want.abs().max())


def _state_len(n, depth=DEPTH):
    return sum((n >> d) ** 2 for d in range(depth))


def _act_weights(weights, act):
    """The state_dict a HybridNet built with ``act`` holds: only PReLU has a slope parameter (pack_weights writes the constant slopes)."""
    return weights if act == "prelu" else {k: v for k, v in weights.items() if not k.endswith("double_conv.1.weight")}


def unet_case(weights, n, b, act="prelu"):
    key = ("unet", n, b, act)
    if key not in _cache:
        g = torch.Generator().manual_seed(77 + 13 * n + b + 1000 * ACTS.index(act))
        x = torch.randn(b, 6, n, n, generator=g, dtype=torch.float32).double()
        st = (0.5 * torch.randn(b, 2, _state_len(n), generator=g, dtype=torch.float32)).double()     # non-zero: zeros hide a swapped concatenation
        w64 = {k: v.double() for k, v in _act_weights(weights, act).items()}
        d, new = O.unet_forward(x, O.unflatten_states(st, n, DEPTH), w64, DEPTH, act)
        assert d.dtype == torch.float64
        _cache[key] = dict(x=x, st=st, d=d, new=new)
    return _cache[key]


def step_case(weights, n, b, sb):
    """Ten iterations of O.single_step from O.solve's start (wavefield and states zero), every intermediate kept."""
    key = ("step", n, b, sb)
    if key not in _cache:
        g = torch.Generator().manual_seed(500 + n + 10 * b + sb)
        sos = (1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float32)).double()
        src = torch.cat([O.point_source_map(n, [n // 2 + 3 * i, n // 3 + i], 10.0) for i in range(sb)], 0).float().double().contiguous()   # (point_source_map returns a permuted view)
        t64 = O.SpectralTables(n, PML, SIGMA_MAX, K, dtype=torch.float64)
        w64 = {k: v.double() for k, v in weights.items()}
        k_sq, wf = O.get_initials(sos, 1.0)
        states = [torch.zeros(b, 2, s, s, dtype=torch.float64) for s in O.state_dims(n, DEPTH)]
        res = O.get_residual(wf, k_sq, src, t64)
        c = dict(k_sq=k_sq, src=src, wf0=wf, res0=res.contiguous(), st0=O.flatten_states(states), wf=[], res=[], st=[], rmse=[])
        for _ in range(N_ITER):
            wf, res, states = O.single_step(wf, k_sq, res, states, w64, src, t64, DEPTH)
            c["wf"].append(wf)
            c["res"].append(res)
            c["st"].append(O.flatten_states(states))
            c["rmse"].append(O.test_loss_function(res))
        assert wf.dtype == res.dtype == torch.float64
        _cache[key] = c
    return _cache[key]


def _engine(weights, act="prelu"):
    from helmnet_amd.engine import Engine, pack_weights
    e = Engine(DEV)
    e.load_weights(pack_weights(_act_weights(weights, act), DEPTH, act), 8, DEPTH, 2, act)
    return e


@pytest.fixture(scope="module")
def eng(weights):
    e = _engine(weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    return s


def _check_unet(e, c, n, tag):
    d, new = e.unet64(c["x"].to(DEV), c["st"].to(DEV))
    assert d.dtype == new.dtype == torch.float64
    errs = [_rel(d, c["d"])] + [_rel(got, want) for got, want in zip(O.unflatten_states(new, n, DEPTH), c["new"])]
    print(f"{tag}: d {errs[0]:.3e}, new states by level {['%.3e' % v for v in errs[1:]]} (of max|expected|)")
    assert max(errs) <= BAR_UNET, errs
    return d, new


# ---------------------------------------------------------------------------------------------- 1: hn_unet_f64 against the oracle
@pytest.mark.parametrize("n,b", UNET_CASES)
def test_unet_matches_the_float64_oracle(eng, weights, n, b):
    eng.set_domain(n, PML, SIGMA_MAX, K)
    c = unet_case(weights, n, b)
    d, new = _check_unet(eng, c, n, f"n={n} b={b}")
    d2, new2 = eng.unet64(c["x"].to(DEV), c["st"].to(DEV))
    assert torch.equal(d, d2) and torch.equal(new, new2)


def test_unet_is_float64_and_not_a_cast(eng, weights):
    """The fp32 hn_unet of the same (fp32-representable) inputs is at least 1e3 times farther from the float64 oracle."""
    eng.set_domain(96, PML, SIGMA_MAX, K)
    c = unet_case(weights, 96, 1)
    d64, _ = eng.unet64(c["x"].to(DEV), c["st"].to(DEV))
    d32, _ = eng.unet(c["x"].float().to(DEV), c["st"].float().to(DEV))
    e64, e32 = _rel(d64, c["d"]), _rel(d32.double(), c["d"])
    print(f"n=96: float64 path {e64:.3e}, fp32 path {e32:.3e} of max|expected|")
    assert e64 * 1e3 <= e32


# ---------------------------------------------------------------------------------------------- 2: every activation, and levels without state
@pytest.mark.parametrize("act", ACTS)
def test_unet_every_activation(weights, act):
    e = _engine(weights, act)
    try:
        e.set_domain(32, PML, SIGMA_MAX, K)
        _check_unet(e, unet_case(weights, 32, 2, act), 32, act)
    finally:
        e.close()


def test_levels_without_state_keep_their_slots_bit_for_bit(hparams):
    """depth 4 / state_depth 2 (random weights of the reference-made fixture) through IterativeSolver.n_steps64: one iteration against O.single_step, and
    the slots of levels 2, 3 in the final states and in the state history are the bits that went in."""
    from helmnet_amd import IterativeSolver
    with np.load(os.path.join(REPO, "tests", "golden", "r2_state_depth.npz")) as z:
        w = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}
    n, b = 64, 2
    s = IterativeSolver(**{**hparams, "domain_size": n, "state_depth": 2})
    s.f.load_state_dict(w, strict=True)
    s.freeze()
    s.to(DEV)
    g = torch.Generator().manual_seed(64)
    wf = (0.1 * torch.randn(b, 2, n, n, generator=g, dtype=torch.float32)).double()
    sos = (1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float32)).double()
    st = (0.5 * torch.randn(b, 2, _state_len(n), generator=g, dtype=torch.float32)).double()
    k_sq = (1.0 / sos) ** 2
    hp = s.hparams
    t64 = O.SpectralTables(n, int(hp.PMLsize), float(hp.sigma_max), float(hp.k), dtype=torch.float64)
    src = s.source.detach().double().cpu()
    res = O.get_residual(wf, k_sq, src, t64).contiguous()
    want_wf, want_res, want_st = O.single_step(wf, k_sq, res, O.unflatten_states(st, n, DEPTH), {k: v.double() for k, v in w.items()}, src, t64, DEPTH,
                                               state_depth=2)
    out = s.n_steps64(wf.to(DEV), k_sq.to(DEV), res.to(DEV), st.to(DEV), 1, return_states=True, residuals="last")
    a = sum((n >> d) ** 2 for d in range(2))
    for got in (out["final_states"], out["states"][0]):
        assert torch.equal(got[:, :, a:].cpu(), st[:, :, a:])
        errs = [_rel(x, y) for x, y in zip(O.unflatten_states(got, n, DEPTH)[:2], want_st[:2])]
        assert max(errs) <= BAR_UNET, errs
    e_wf, e_res = _rel(out["wavefields"][0], want_wf), _rel(out["residuals"][0], want_res)
    print(f"state_depth 2: wavefield {e_wf:.3e}, residual {e_res:.3e}, states {errs} of max|expected|")
    assert e_wf <= BAR_UNET and e_res <= BAR_STEP


# ---------------------------------------------------------------------------------------------- 3: hn_step_f64 plumbing
def _run_step(e, c, b, n_iter=N_ITER, hist=True):
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV, dtype=torch.float64)  # noqa: E731
    n = c["wf0"].shape[-1]
    wf, res, st = c["wf0"].to(DEV).clone(), c["res0"].to(DEV).clone(), c["st0"].to(DEV).clone()
    h = dict(res_hist=new(n_iter, b, 2, n, n), wf_hist=new(n_iter, b, 2, n, n), st_hist=new(n_iter, b, 2, st.shape[-1]), rmse_hist=new(n_iter, b)) if hist else {}
    e.step64(wf, res, st, c["k_sq"].to(DEV), c["src"].to(DEV), n_iter, **h)
    return wf, res, st, h


@pytest.mark.parametrize("n,b,sb", STEP_CASES)
def test_step_matches_ten_oracle_iterations(eng, weights, n, b, sb):
    eng.set_domain(n, PML, SIGMA_MAX, K)
    c = step_case(weights, n, b, sb)
    wf, res, st, h = _run_step(eng, c, b)
    errs = {"wf": _rel(wf, c["wf"][-1]), "res": _rel(res, c["res"][-1]), "st": _rel(st, c["st"][-1])}
    for it in range(N_ITER):
        errs[f"wf_hist[{it}]"] = _rel(h["wf_hist"][it], c["wf"][it])
        errs[f"res_hist[{it}]"] = _rel(h["res_hist"][it], c["res"][it])
        errs[f"st_hist[{it}]"] = _rel(h["st_hist"][it], c["st"][it])
        errs[f"rmse_hist[{it}]"] = float(((h["rmse_hist"][it].cpu() - c["rmse"][it]).abs() / c["rmse"][it]).max())
    worst = max(errs, key=errs.get)
    print(f"n={n} b={b} src_batch={sb}: final wf {errs['wf']:.3e} res {errs['res']:.3e} states {errs['st']:.3e}; worst {worst} {errs[worst]:.3e} (of max|expected|)")
    assert errs[worst] <= BAR_STEP, (worst, errs[worst])
    # the final tensors are the last history slots, and a run without histories or with an odd iteration count gives the same bits
    assert torch.equal(wf, h["wf_hist"][-1]) and torch.equal(res, h["res_hist"][-1]) and torch.equal(st, h["st_hist"][-1])
    wf2, res2, st2, h2 = _run_step(eng, c, b)
    assert torch.equal(wf, wf2) and torch.equal(res, res2) and torch.equal(st, st2) and all(torch.equal(h[k], h2[k]) for k in h)
    wf3, res3, st3, _ = _run_step(eng, c, b, n_iter=3, hist=False)
    assert torch.equal(wf3, h["wf_hist"][2]) and torch.equal(res3, h["res_hist"][2]) and torch.equal(st3, h["st_hist"][2])


def test_step_argument_and_state_errors(eng, weights):
    from helmnet_amd.engine import Engine
    n, b = 16, 1
    eng.set_domain(n, PML, SIGMA_MAX, K)
    c = step_case(weights, n, b, 1)
    lib, stream = eng.lib, eng._stream()
    wf, res, st = c["wf0"].to(DEV).clone(), c["res0"].to(DEV).clone(), c["st0"].to(DEV).clone()
    k_sq, src = c["k_sq"].to(DEV), c["src"].to(DEV)
    both = torch.zeros(2 * wf.numel(), device=DEV, dtype=torch.float64)
    hist = torch.empty(2, b, 2, n, n, device=DEV, dtype=torch.float64)
    st_hist = torch.empty(2, b, 2, st.shape[-1], device=DEV, dtype=torch.float64)

    def call(wf_=wf, res_=res, st_=st, res_hist=None, wf_hist=None, st_hist_=None, rmse=None, sb=1, ctx=eng.ctx):
        return lib.hn_step_f64(ctx, _ptr(wf_), _ptr(res_), _ptr(st_), _ptr(k_sq), _ptr(src), sb, b, 2, _ptr(res_hist), _ptr(wf_hist), _ptr(st_hist_),
                               _ptr(rmse), stream)

    assert call(wf_=None) == -1
    assert call(res_=wf) == -1                                         # res is wf
    assert call(wf_=both[: wf.numel()], res_=both[wf.numel() // 2: wf.numel() // 2 + wf.numel()]) == -1   # res overlaps half of wf
    assert call(st_hist_=st) == -1                                     # the state history aliases the states
    assert call(wf_hist=hist, res_hist=hist) == -1                     # two histories in one buffer
    assert call(wf_hist=hist, rmse=hist.view(-1)[8:]) == -1            # rmse_hist inside wf_hist
    assert call(res_hist=hist, wf_=hist[1]) == -1                      # wf is a slot of the residual history
    assert call(sb=3) == -1                                            # src_batch neither 1 nor B
    assert lib.hn_unet_f64(eng.ctx, _ptr(both), _ptr(st), _ptr(st), _ptr(wf), b, stream) == -1       # states_in is states_out
    assert "states_in overlaps states_out" in lib.hn_last_error(eng.ctx).decode()
    in6 = torch.zeros(b, 6, n, n, device=DEV, dtype=torch.float64)
    assert lib.hn_unet_f64(eng.ctx, _ptr(in6), _ptr(in6.view(-1)[: st.numel()]), _ptr(torch.empty_like(st)), _ptr(torch.empty_like(wf)), b, stream) == 0   # read against read
    assert call() == 0
    with pytest.raises(TypeError):
        eng.step64(wf.float(), res, st, k_sq, src, 1)
    with pytest.raises(ValueError):
        eng.step64(wf, res, st[:, :, :-1].contiguous(), k_sq, src, 1)
    with pytest.raises(TypeError):
        eng.unet64(torch.zeros(b, 6, n, n, device=DEV), st)
    fresh = Engine(DEV)                                                # neither weights nor domain
    try:
        assert call(ctx=fresh.ctx) == -2
        fresh.set_domain(n, PML, SIGMA_MAX, K)
        assert call(ctx=fresh.ctx) == -2                               # still no weights
        assert lib.hn_unet_f64(fresh.ctx, _ptr(both), _ptr(st), _ptr(st_hist), _ptr(wf), b, stream) == -2
    finally:
        fresh.close()
    torch.cuda.synchronize()


def test_step_is_capturable_once_its_buffers_exist(eng, weights):
    n, b, sb = 48, 2, 2
    c = step_case(weights, n, b, sb)
    eng.set_domain(16, PML, SIGMA_MAX, K)
    eng.set_domain(n, PML, SIGMA_MAX, K)                               # a fresh domain: no float64 weights, workspace or tables yet
    k_sq, src = c["k_sq"].to(DEV), c["src"].to(DEV)
    wf, res, st = c["wf0"].to(DEV).clone(), c["res0"].to(DEV).clone(), c["st0"].to(DEV).clone()
    wf_hist = torch.empty(3, b, 2, n, n, device=DEV, dtype=torch.float64)
    rmse = torch.empty(3, b, device=DEV, dtype=torch.float64)

    def call():
        return eng.lib.hn_step_f64(eng.ctx, _ptr(wf), _ptr(res), _ptr(st), _ptr(k_sq), _ptr(src), sb, b, 3, None, _ptr(wf_hist), None, _ptr(rmse), eng._stream())

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rmse.zero_()
            rc = call()
        assert rc == -2                                                # would have to build: refused before anything is enqueued, the capture ends in order
        want_wf, want_res, want_st, _ = _run_step(eng, c, b, n_iter=3)     # eager, with an RMSE history: builds everything
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = call()
        assert rc == 0
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(wf, want_wf) and torch.equal(res, want_res) and torch.equal(st, want_st)
    assert torch.equal(wf_hist[-1], want_wf) and _rel(wf_hist[0], c["wf"][0]) <= BAR_STEP
    assert float(((rmse.cpu() - torch.stack(c["rmse"][:3])).abs() / torch.stack(c["rmse"][:3])).max()) <= BAR_STEP


def _first_sample(c):
    """The batch-1 problem that is sample 0 of a step_case with one source."""
    return {k: c[k][:1].contiguous() for k in ("wf0", "res0", "st0", "k_sq", "src")}


def _same_run(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and all(torch.equal(a[3][k], b[3][k]) for k in a[3])


# n = 16: one (partial) 32 x 32 tile of the residual per sample; 48: four, three of them partial
@pytest.mark.parametrize("n", [16, 48])
def test_step_workspace_grown_then_reused_by_a_smaller_batch(eng, weights, n):
    """Batch 1, 2, 1 on one context: the workspace, the second state buffer and the partial sums are built for one sample, grown for two, and the
    batch-1 call in buffers sized for two gives the bits of the call that built them -- as does a rebuild after hn_set_domain has freed everything."""
    c2 = step_case(weights, n, 2, 1)
    c1 = _first_sample(c2)
    eng.set_domain(16, PML, SIGMA_MAX, K)
    eng.set_domain(n, PML, SIGMA_MAX, K)                               # a fresh domain: no float64 weights, workspace or tables yet
    first = _run_step(eng, c1, 1, n_iter=2)
    big = _run_step(eng, c2, 2, n_iter=2)
    last = _run_step(eng, c1, 1, n_iter=2)
    assert bool(torch.isfinite(first[3]["rmse_hist"]).all()) and _same_run(first, last)
    assert all(torch.equal(x[:1], y) for x, y in zip(big[:3], first[:3])) and torch.equal(big[3]["rmse_hist"][:, :1], first[3]["rmse_hist"])
    eng.set_domain(16, PML, SIGMA_MAX, K)
    eng.set_domain(n, PML, SIGMA_MAX, K)                               # frees and rebuilds
    assert _same_run(first, _run_step(eng, c1, 1, n_iter=2))


def test_captured_step_needs_the_partial_sums_only_with_an_rmse_history(eng, weights):
    """The float64 weights, a workspace for two samples and the float64 tables exist, the partial sums are sized for ONE sample: a captured batch-2
    call without an RMSE history has nothing to build and replays to the eager bits, one with an RMSE history is refused before it enqueues anything."""
    n, b = 48, 2
    c2 = step_case(weights, n, b, 1)
    eng.set_domain(16, PML, SIGMA_MAX, K)
    eng.set_domain(n, PML, SIGMA_MAX, K)
    _run_step(eng, _first_sample(c2), 1, n_iter=1)                     # eager, batch 1, with an RMSE history: partial sums for one sample
    want_wf, want_res, want_st, _ = _run_step(eng, c2, b, n_iter=3, hist=False)   # eager, batch 2, no RMSE: grows the workspace, not the partial sums
    k_sq, src = c2["k_sq"].to(DEV), c2["src"].to(DEV)
    wf, res, st = c2["wf0"].to(DEV).clone(), c2["res0"].to(DEV).clone(), c2["st0"].to(DEV).clone()
    rmse = torch.full((3, b), -7.0, device=DEV, dtype=torch.float64)
    probe = torch.zeros(4, device=DEV)

    def call(rmse_hist):
        return eng.lib.hn_step_f64(eng.ctx, _ptr(wf), _ptr(res), _ptr(st), _ptr(k_sq), _ptr(src), 1, b, 3, None, None, None, _ptr(rmse_hist), eng._stream())

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            probe.add_(1.0)
            rc = call(rmse)
        assert rc == -2 and "capture" in eng.lib.hn_last_error(eng.ctx).decode()
        graph.replay()                                                 # the capture ended in order and holds nothing of the library's
        torch.cuda.synchronize()
        assert probe.tolist() == [1.0] * 4 and torch.equal(wf, c2["wf0"].to(DEV)) and bool((rmse == -7.0).all())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = call(None)
        assert rc == 0
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(wf, want_wf) and torch.equal(res, want_res) and torch.equal(st, want_st)


# ---------------------------------------------------------------------------------------------- 4: the reference's own float64 trajectory
def test_forward64_follows_the_reference_float64_trajectory(solver):
    with np.load(os.path.join(REPO, "tests", "golden", "long_run.npz")) as z:
        g = {k: z[k] for k in ("cfg2_stride", "cfg2_wf_it100", "cfg2_rmse_f64")}
    li = long_inputs("cfg2")
    solver.set_domain_size(256, source_location=list(li["loc"]))
    torch.set_default_dtype(torch.float64)   # the reference's float64 run builds its source map under this default
    try:
        src = O.point_source_map(256, li["loc"], 10.0)
    finally:
        torch.set_default_dtype(torch.float32)
    assert src.dtype == torch.float64
    out = solver.forward64(torch.from_numpy(li["sos"][1:2]).to(DEV), num_iterations=100, residuals="norms", source=src.to(DEV))
    st = int(g["cfg2_stride"])
    gold = g["cfg2_wf_it100"][1:2].astype(np.float64)
    got = out["wavefields"][0].cpu().numpy()[:, :, ::st, ::st]
    err, scale = np.abs(got - gold).max(), np.abs(gold).max()
    trace = out["residual_norms"].cpu().numpy()
    rel = np.abs(trace / g["cfg2_rmse_f64"][:100, 1:2] - 1).max()
    print(f"100 iterations at 256^2: wavefield {err / scale:.3e} of the largest probe value, RMSE trace {rel:.3e} relative")
    assert out["wavefields"][0].dtype == torch.float64 and trace.shape == (100, 1)
    assert err <= 1e-7 * scale, (err, scale)
    assert rel <= 1e-6


# ---------------------------------------------------------------------------------------------- 5: the same problem as the fp32 path
def test_forward64_solves_the_problem_forward_solves(solver):
    from helmnet_amd.phantoms import ring_sos_batch
    solver.set_domain_size(96, source_location=[82, 48])
    sos = torch.from_numpy(ring_sos_batch(96, 2, seed=5)).to(DEV)
    o32 = solver.forward(sos, num_iterations=20, residuals="norms")
    held = [e.state.clone() for e in solver.f.enc]
    o64 = solver.forward64(sos, num_iterations=20, return_wavefields=True, return_states=True, residuals="all")
    assert all(torch.equal(e.state, h) and e.state.dtype == torch.float32 for e, h in zip(solver.f.enc, held))   # f's fp32 states: untouched
    assert set(o64) == set(solver.forward(sos, num_iterations=2, return_wavefields=True, return_states=True, residuals="all"))
    assert len(o64["wavefields"]) == len(o64["residuals"]) == len(o64["states"]) == 20 and o64["last_iteration"] == 19
    assert all(t.dtype == torch.float64 for t in o64["wavefields"] + o64["residuals"] + o64["states"] + [o64["residual_norms"]])
    apart = float((o32["wavefields"][0].double() - o64["wavefields"][-1]).abs().max())
    print(f"n=96, 20 iterations: |forward - forward64| = {apart:.3e}")
    assert apart <= 1e-4
    dev = solver.deviation_from_float64(sos, 20, [5, 10, 20])
    assert set(dev) == {"iterations", "linf", "rmse32", "rmse64"}
    assert dev["iterations"].tolist() == [5, 10, 20] and dev["linf"].shape == (3, 2) and dev["linf"].dtype == torch.float64
    assert dev["rmse32"].shape == (20, 2) and dev["rmse64"].shape == (20, 2) and dev["rmse64"].dtype == torch.float64
    assert all(bool(torch.isfinite(dev[k]).all()) for k in ("linf", "rmse32", "rmse64"))
    assert torch.equal(dev["rmse64"], o64["residual_norms"])           # chunked or whole: the float64 loop gives the same bits
    assert float(dev["linf"].max()) <= 1e-4                            # the fp32 wavefield bar holds at every checkpoint of these 20 iterations
    print(f"deviation_from_float64: linf {dev['linf'].tolist()}")
    with pytest.raises(RuntimeError):
        solver.forward64(sos.clone().requires_grad_(True), num_iterations=1)
    with pytest.raises(ValueError):
        solver.forward64(sos, num_iterations=1, source=solver.source.detach())      # an fp32 source map
