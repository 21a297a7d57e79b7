"""Every form of the hn_step loop (tests/loop_forms.py) on a real MI355X.

The PLAIN form -- no side stream, no capture, copied histories, one call per iteration -- is measured against the float64 oracle looped on a CPU
(classes B, C, D; A and E are anchored by the teacher-forced float64 rows of tests/test_config_matrix.py: one step, the same kernels).  Every
other row must give the plain form's bits in wf, res, the hidden states and every history slot it asks for, its rmse_hist within the bar of the
float atomics, twice on one context and once more as two calls of a + b iterations with a odd; around every call the deltas of graph_replays,
eager_iterations, graphs_captured and flag_sync_iterations are those loop_forms.expected_counters derives from the header -- a form that silently
fell back to another (a capture that failed, device words that never engaged) changes them.

The inputs are config_input(wf_scale=0.5) with a point source: the seeded networks are no contraction, so the fields grow by about 4.6 x per
iteration (to 1e5 after 9 iterations, 2e11 after 18), which costs the comparison nothing: every bar is relative.

Measured on an MI355X (plain form, 9 iterations, samples 0 and b - 1, relative to max |float64| of the tensor; in brackets the CPU oracle in fp32
against itself in float64):
  B d3_128, HN_OPT_DEEP 1   wf 4.49e-06 (4.99e-06)   states 7.02e-06 (8.07e-06), 9.81e-06 (1.24e-05), 8.62e-06 (9.68e-06)
  C 96^2 depth 4            wf 4.95e-06 (7.23e-06)   states 6.84e-06 (1.22e-05), 1.69e-06 (3.08e-06), 6.65e-06 (8.22e-06), 4.48e-06 (4.16e-06)
  D d2_64                   wf 3.18e-06 (4.13e-06)   states 3.61e-06 (4.33e-06), 4.55e-06 (6.51e-06)
Bars: wf <= max(1e-4, 2 x oracle) and <= 4e-4; a state level 1e-5, or 2 x the oracle where that is above 5e-6.  All 55 rows gave the plain
form's bits and the model's counters; a whole row (plain reference included) takes 0.02 .. 0.7 s.
"""
import pytest
import torch

import loop_forms as LF
from config_solver import DEV, _solver
from config_weights import config_input, config_weights
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

_CASES, _PLAIN = {}, {}


def _case(cls):
    """The class's network and inputs (host tensors), built once."""
    if cls not in _CASES:
        (depth, seed, plan, act, sd), n, b = LF.CLASSES[cls]
        w = config_weights(depth, seed, plan, act, sd, n=n)
        x = {k: torch.from_numpy(v) for k, v in config_input(n, b, depth, LF.INPUT_SEED + n, wf_scale=0.5).items()}
        k_sq, _ = O.get_initials(x["sos"], 1.0)
        _CASES[cls] = dict(depth=depth, act=act, sd=sd, n=n, b=b, w=w, wf=x["wf"], res=x["res"], states=x["states"], k_sq=k_sq.contiguous(),
                           src=O.point_source_map(n, [n // 8, n // 2], 10.0).contiguous())
    return _CASES[cls]


def _engine(c, precision, fixed, form):
    s = _solver(c["depth"], c["act"], c["sd"], c["w"], c["n"], mode=None if precision == "fp32" else precision, zero_source=False)
    eng = s.engine()
    for k, v in list(fixed.items()) + list(form.items()):
        eng.set_option(k, v)
    return s, eng           # (the solver owns the engine: keep it alive)


def _buffers(c, eng, n_iter, histories):
    b, n = c["b"], c["n"]
    t = {k: c[k].to(DEV).contiguous() for k in ("wf", "res", "states")}
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)      # noqa: E731
    t["res_hist"] = nan(n_iter, b, 2, n, n) if "res" in histories else None
    t["wf_hist"] = nan(n_iter, b, 2, n, n) if "wf" in histories else None
    t["st_hist"] = nan(n_iter, b, 2, eng.state_len) if "st" in histories else None
    t["rmse_hist"] = nan(n_iter, b) if "rmse" in histories else None
    return t


def _refill(c, t):
    for k in ("wf", "res", "states"):
        t[k].copy_(c[k])
    for k in ("res_hist", "wf_hist", "st_hist", "rmse_hist"):
        if t[k] is not None:
            t[k].fill_(float("nan"))


def _counters(eng):
    return {k: eng.counter(k) for k in LF.COUNTERS}


def _call(eng, t, dev, i0, i1, expect, what):
    """Iterations [i0, i1) of the row as ONE hn_step call on the slices of the histories; the counters must move as ``expect`` says."""
    sl = lambda h: None if h is None else h[i0:i1]        # noqa: E731
    c0 = _counters(eng)
    eng.step(t["wf"], t["res"], t["states"], dev["k_sq"], dev["src"], i1 - i0, sl(t["res_hist"]), sl(t["wf_hist"]), sl(t["st_hist"]), sl(t["rmse_hist"]))
    torch.cuda.synchronize()
    c1 = _counters(eng)
    delta = {k: c1[k] - c0[k] for k in LF.COUNTERS}
    assert delta == expect, (what, delta, expect)


def _plain(cls, precision, fixed, n_iter):
    """The plain form of (class, precision, fixed options): every iteration's wf, res, states and rmse, as n_iter calls of one iteration."""
    key = (cls, precision, tuple(sorted(fixed.items())))
    if key in _PLAIN and _PLAIN[key]["rmse_hist"].shape[0] >= n_iter:
        return _PLAIN[key]
    c = _case(cls)
    s, eng = _engine(c, precision, fixed, LF.PLAIN)
    dev = {k: c[k].to(DEV) for k in ("k_sq", "src")}
    t = _buffers(c, eng, n_iter, LF.HISTORIES)
    one = LF.expected_counters(LF.PLAIN, precision, 1, c["b"], LF.HISTORIES)
    for it in range(n_iter):
        _call(eng, t, dev, it, it + 1, one, f"plain {key} iteration {it}")
    eng.check_async_errors()
    for k in ("res_hist", "wf_hist", "st_hist", "rmse_hist"):
        assert torch.isfinite(t[k]).all(), k
    assert torch.equal(t["wf"], t["wf_hist"][-1]) and torch.equal(t["res"], t["res_hist"][-1]) and torch.equal(t["states"], t["st_hist"][-1])
    if precision == "fp32":      # the class reaches the route it is there for (one more iteration, its kernels bracketed)
        must, must_not = LF.ROUTES[cls, fixed.get("deep", 2)]
        eng.profile_enable(None)
        eng.step(t["wf"].clone(), t["res"].clone(), t["states"].clone(), dev["k_sq"], dev["src"], 1)
        torch.cuda.synchronize()
        names = set(eng.profile_collect())
        eng.profile_enable([])
        eng.check_async_errors()
        assert must <= names and not (must_not & names), (key, sorted(names))
    _PLAIN[key] = {k: t[k] for k in ("res_hist", "wf_hist", "st_hist", "rmse_hist")}
    return _PLAIN[key]


def _rmse64(res):
    return res.double().pow(2).mean(dim=(-3, -2, -1)).sqrt()


def _same(what, t, ref, i0, i1, histories, final=True):
    """Bit for bit the plain form's iterations [i0, i1): the live buffers hold iteration i1 - 1, every asked-for history slot its iteration."""
    if final:
        for k, h in (("wf", "wf_hist"), ("res", "res_hist"), ("states", "st_hist")):
            assert torch.equal(t[k], ref[h][i1 - 1]), (what, k, i1)
    for name, h in (("res", "res_hist"), ("wf", "wf_hist"), ("st", "st_hist")):
        if name in histories:
            for it in range(i0, i1):
                assert torch.equal(t[h][it], ref[h][it]), (what, h, it)
    if "rmse" in histories:
        got = t["rmse_hist"][i0:i1]
        # sums of squares added up with float atomics: order-dependent in the last bits (the project's bar for them)
        assert torch.allclose(got, ref["rmse_hist"][i0:i1], rtol=1e-5, atol=0), (what, "rmse_hist", got, ref["rmse_hist"][i0:i1])
        if "res" in histories:      # and it IS the RMSE of the residual the same call returned (2 n^2 >= 8192 non-negative fp32 terms summed in blocks)
            want = _rmse64(t["res_hist"][i0:i1])
            assert torch.allclose(got.double(), want, rtol=1e-5, atol=0), (what, "rmse vs res_hist", got, want)


@pytest.mark.parametrize("row", LF.ROWS, ids=[r[0] for r in LF.ROWS])
def test_form_gives_the_plain_form_bit_for_bit(row):
    tag, _, n, b, precision, fixed, form, n_iter, histories = row
    cls = LF.row_class(row)
    c = _case(cls)
    ref = _plain(cls, precision, fixed, n_iter)
    s, eng = _engine(c, precision, fixed, form)
    dev = {k: c[k].to(DEV) for k in ("k_sq", "src")}
    # twice on one context, on the same buffers: epochs, graph cache and counters continue across the calls
    t = _buffers(c, eng, n_iter, histories)
    for rep in (0, 1):
        if rep:
            _refill(c, t)
        _call(eng, t, dev, 0, n_iter, LF.expected_counters(form, precision, n_iter, b, histories, cached=bool(rep)), f"{tag} run {rep}")
        _same(f"{tag} run {rep}", t, ref, 0, n_iter, histories)
    # a + b iterations in two calls, a odd: the first call must leave the states in the caller's buffer
    a = LF.split_point(n_iter)
    t2 = _buffers(c, eng, n_iter, histories)
    first = LF.expected_counters(form, precision, a, b, histories)
    _call(eng, t2, dev, 0, a, first, f"{tag} first {a}")
    _same(f"{tag} first {a}", t2, ref, 0, a, histories)
    # (the second call's graph is the first's, if that captured one, unless the rmse_hist slice moved: the cache is keyed on the pointers)
    cached = first["graphs_captured"] == 1 and "rmse" not in histories
    _call(eng, t2, dev, a, n_iter, LF.expected_counters(form, precision, n_iter - a, b, histories, cached=cached), f"{tag} last {n_iter - a}")
    _same(f"{tag} last {n_iter - a}", t2, ref, a, n_iter, histories)
    _same(f"{tag} first {a}, afterwards", t2, ref, 0, a, histories, final=False)      # the second call left the first call's slots alone
    eng.check_async_errors()
    if precision == "valu":
        # the direct kernels: HN_OPT_DEEP / HN_OPT_DC_PAIR have no effect, every level runs layer by layer
        eng.profile_enable(None)
        _refill(c, t)
        eng.step(t["wf"], t["res"], t["states"], dev["k_sq"], dev["src"], 1)
        torch.cuda.synchronize()
        names = set(eng.profile_collect())
        eng.profile_enable([])
        eng.check_async_errors()
        assert not ({"deep", "inc_conv_signal0"} & names), sorted(names)
        assert {"inc", "bottleneck"} | {f"conv_signal{d}" for d in range(c["depth"])} <= names, sorted(names)
        assert torch.equal(t["wf"], ref["wf_hist"][0]) and torch.equal(t["states"], ref["st_hist"][0])


def _oracle_loop(c, dtype, idx, n_iter):
    w = {k: torch.from_numpy(v).to(dtype) for k, v in c["w"].items()}
    n, depth = c["n"], c["depth"]
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=dtype)
    wf, res, k_sq, src = c["wf"][idx].to(dtype), c["res"][idx].to(dtype), c["k_sq"][idx].to(dtype), c["src"].to(dtype)
    st = O.unflatten_states(c["states"][idx].to(dtype), n, depth)
    for _ in range(n_iter):
        wf, res, st = O.single_step(wf, k_sq, res, st, w, src, t, depth, c["act"], state_depth=c["sd"])
    return wf, O.flatten_states(st)


@pytest.mark.parametrize("row", LF.PLAIN_ROWS, ids=[r[0] for r in LF.PLAIN_ROWS])
def test_plain_form_vs_float64(row):
    """The anchor of the matrix: the plain form's free-running loop against the float64 oracle, with the bar of
    test_config_matrix.py::test_loop_is_repeated_single_step_bit_for_bit for the wavefield and each level's final hidden state on its own scale
    in the _vs_float64 form."""
    tag, _, n, b, precision, fixed, form, n_iter, histories = row
    assert form == LF.PLAIN
    cls = LF.row_class(row)
    c = _case(cls)
    ref = _plain(cls, precision, fixed, n_iter)
    idx = [0, b - 1]
    wf64, st64 = _oracle_loop(c, torch.float64, idx, n_iter)
    wf32, st32 = _oracle_loop(c, torch.float32, idx, n_iter)
    wf = ref["wf_hist"][n_iter - 1][idx].cpu().double()
    scale = wf64.abs().max().item()
    err, ora = (wf - wf64).abs().max().item(), (wf32.double() - wf64).abs().max().item()
    report = [f"wf {err / scale:.2e} (fp32 oracle {ora / scale:.2e})"]
    ok = [err <= max(1e-4 * scale, 2 * ora) and err <= 4e-4 * scale]
    o = 0
    for d in range(c["depth"]):
        lv = slice(o, o + (n >> d) ** 2)
        o += (n >> d) ** 2
        g, w64, w32 = ref["st_hist"][n_iter - 1][idx][:, :, lv].cpu().double(), st64[:, :, lv], st32[:, :, lv].double()
        sc = w64.abs().max().item()
        e, r = (g - w64).abs().max().item() / sc, (w32 - w64).abs().max().item() / sc
        bar = 1e-5 if r <= 5e-6 else 2 * r
        report.append(f"state{d} {e:.2e} (fp32 oracle {r:.2e}, bar {bar:.2e})")
        ok.append(e <= bar)
    print(f"[{tag}] {n_iter} it, |wf| {scale:.3e}: " + "; ".join(report))
    assert all(ok), report
