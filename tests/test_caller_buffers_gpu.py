"""Every entry point on caller buffers that are only element-aligned (carved out of larger allocations) or that overlap.  Needs a real MI355X.

include/helmnet_hip.h ("alignment and overlap") promises that a tensor needs the alignment of its element type and no more, unless the entry
point names one.  DESIGN.md ("Caller buffers: alignment and overlap") lists, per entry point and argument, the widest access the kernels make
on the caller's pointer, its guard, and the route a pointer that is only 4-byte aligned takes: two routes stand down (hn_dca.hip and hn_cs.hip,
whose LDS-direct 16-byte loads are guarded by ``dc_asm_applies`` / ``conv_state_applies``), everything else runs the same kernels, whose
float2 / float4 accesses are ordinary vector loads and stores.

Every test here runs its call on plain tensors and on views ``k`` = 1, 2, 3 floats (1 double) past a 16-byte boundary between guard words
(tests/caller_buffers.py) and checks
  (a) every output against the float64 oracle, on the bars the suite already has (``_vs_float64`` of tests/test_config_matrix.py, the
      spectral bar of tests/spectral_probes.py, the float64 bars of tests/test_f64_gpu.py and tests/test_f64_solver_gpu.py, the gradient bars
      of tests/train_matrix.py);
  (b) every output against the plain call: bit for bit where the same kernels run, ``4e-6 * max`` (the bar of tests/test_config_matrix.py
      between kernel sets) where the route changes -- ``_route_changes`` below is the table's last column; offsets 1, 2 and 3 give the same
      bits as each other; sums of float atomics (hn_rmse, rmse_hist, the training loss) cannot be bit-equal between two runs of the same
      kernel and keep the suite's rtol 1e-5 / 1e-6;
  (c) every guard word intact and ``check_async_errors()`` clean.
The profile names confirm the routes: the paired ``inc_conv_signal0`` launch dissolves into ``inc`` and ``conv_signal0`` when wf, res or
states is misaligned, and the merged hidden-state launch (accounted to ``conv_state0``) into one launch per level.

The last section pins the overlap contract of hn_step and hn_unet: refused with HN_ERR_ARG naming both arguments, nothing enqueued; the one
tolerated form is ``res_hist == res`` / ``wf_hist == wf``.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import spectral_probes as SP
import train_matrix as TM
from caller_buffers import Carved
from config_solver import DEV, _solver
from config_weights import config_input, config_weights
from golden_inputs import teacher_inputs
from oracle import helmnet_oracle as O
from test_config_matrix import _levels, _vs_float64

pytestmark = pytest.mark.gpu

KS = (1, 2, 3)
BETWEEN_KERNEL_SETS = 4e-6      # tests/test_config_matrix.py: two kernel sets for the same fp32 arithmetic
NAN = float("nan")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _done(eng, *carved):
    """(c): the stream drained, no device-side wait gave up, every guard word intact."""
    torch.cuda.synchronize()
    eng.check_async_errors()
    for c in carved:
        c.check()


def _same_bits(tag, got, base, keys, atomics=()):
    for k in keys:
        if k in atomics:
            assert torch.allclose(got[k], base[k], rtol=1e-5, atol=0), (tag, k)
        else:
            assert torch.equal(got[k], base[k]), (tag, k, float((got[k] - base[k]).abs().max()))


def _close_or_same(tag, got, base, keys, route_changes, atomics=()):
    """(b).  Prints the measured distance where the bar is not bit-equality."""
    if not route_changes:
        return _same_bits(tag, got, base, keys, atomics)
    worst = {}
    for k in keys:
        if k in atomics:
            assert torch.allclose(got[k], base[k], rtol=1e-5, atol=0), (tag, k)
            continue
        worst[k] = float((got[k] - base[k]).abs().max()) / float(base[k].abs().max())
    print(f"[{tag}] other route, distance to the aligned call / max: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f" (bar {BETWEEN_KERNEL_SETS:.0e})")
    assert all(v <= BETWEEN_KERNEL_SETS for v in worst.values()), (tag, worst)


# =====================================================================================================================================
# 1a. hn_step and hn_unet
# =====================================================================================================================================
# tag -> (depth, weight seed, slope plan, n, batch, precision mode, options, iterations).  256^2 x 2 at depth 4: the smallest size with hn_dca.hip,
# the paired launch and k_deepx; 64^2 at depth 2 (d2_64 of tests/config_weights.py): the smallest with hn_cs.hip; 272^2: partial tiles at every
# level; fp16 / bf16x3 at 256^2 x 1; two lanes need four samples; a captured iteration is replayed from four iterations on (hn_api.hip: n_iter >=
# 4 * per_graph), so that row runs four
NET_CASES = {
    "d4_256": (4, 741, "A", 256, 2, None, {}, 3),
    "d2_64": (2, 744, "B", 64, 2, None, {}, 3),
    "d4_272": (4, 749, "A", 272, 1, None, {}, 3),
    "d4_256_fp16": (4, 741, "A", 256, 1, "fp16", {}, 3),
    "d4_256_bf16x3": (4, 741, "A", 256, 1, "bf16x3", {}, 3),
    "d2_64_lanes2": (2, 744, "B", 64, 4, None, {"lanes": 2}, 3),
    "d2_64_graph": (2, 744, "B", 64, 2, None, {"graph": 1}, 4),
}
LIVE = ("wf", "res", "states", "k_sq", "src")
HIST = ("res_hist", "wf_hist", "st_hist", "rmse_hist")
STEP_OUT = ("wf", "res", "states") + HIST
_net = {}


def _net_case(tag):
    """Solver, inputs, the aligned call's results and the oracle of one row, built once."""
    if tag not in _net:
        depth, seed, plan, n, b, mode, options, iters = NET_CASES[tag]
        w = config_weights(depth, seed, plan, n=n)
        s = _solver(depth, "prelu", depth, w, n, mode=mode)
        eng = s.engine()
        for k, v in options.items():
            eng.set_option(k, v)
        x = config_input(n, b, depth, 9300 + n, wf_scale=1e-6)
        g = torch.Generator().manual_seed(9400 + n)
        L = eng.state_len
        t = {"wf": torch.from_numpy(x["wf"]), "res": torch.from_numpy(x["res"]), "states": torch.from_numpy(x["states"]),
             "k_sq": (1.0 / torch.from_numpy(x["sos"])) ** 2, "src": 1e-3 * torch.randn(1, 2, n, n, generator=g),
             "res_hist": torch.full((iters, b, 2, n, n), NAN), "wf_hist": torch.full((iters, b, 2, n, n), NAN),
             "st_hist": torch.full((iters, b, 2, L), NAN), "rmse_hist": torch.full((iters, b), NAN)}
        u = {"in6": torch.from_numpy(x["x6"]), "states_in": t["states"], "states_out": torch.full((b, 2, L), NAN), "d_out": torch.full((b, 2, n, n), NAN)}
        _net[tag] = dict(depth=depth, n=n, b=b, mode=mode, iters=iters, w=w, s=s, eng=eng, t=t, u=u, L=L,
                         idx=[b - 1] if n >= 256 else [0, b - 1])     # the float64 oracle on a slice of the batch (samples are independent)
    return _net[tag]


def _step_offsets(which, k):
    if which == "aligned":
        return {}
    if which == "hist":
        return {h: k for h in HIST}
    if which == "all":
        return {name: k for name in LIVE + HIST}
    return {which: k}


def _run_step(c, offsets, iters=None, hist=True, profile=False):
    """One hn_step call on fresh copies of the row's inputs -> (the carved set, the profile names if asked for)."""
    eng = c["eng"]
    iters = c["iters"] if iters is None else iters
    t = dict(c["t"])
    for h in HIST:
        t[h] = t[h][:iters] if hist else None
    cv = Carved(t, DEV, offsets)
    if profile:
        eng.profile_enable(None)
    eng.step(*[cv[k] for k in LIVE], iters, *[cv[h] for h in HIST])
    _done(eng, cv)
    names = None
    if profile:
        names = set(eng.profile_collect())
        eng.profile_enable([])
    return cv, names


def _step_oracle(c, dtype):
    key = ("step_oracle", dtype)
    if key not in c:
        n, depth, idx = c["n"], c["depth"], c["idx"]
        w = {k: torch.from_numpy(v).to(dtype) for k, v in c["w"].items()}
        t = c["t"]
        tab = O.SpectralTables(n, 8, 2, 1.0, dtype=dtype)
        wf, res, k_sq, src = t["wf"][idx].to(dtype), t["res"][idx].to(dtype), t["k_sq"][idx].to(dtype), t["src"].to(dtype)
        st = O.unflatten_states(t["states"][idx].to(dtype), n, depth)
        rows = []
        for _ in range(c["iters"]):
            wf, res, st = O.single_step(wf, k_sq, res, st, w, src, tab, depth, "prelu")
            rows.append((wf, res, O.flatten_states(st)))
        c[key] = rows
    return c[key]


def _step_vs_float64(tag, c, cv):
    """(a): every history row and the final tensors of an fp32 row against the float64 oracle; the states level by level (each on its own scale)."""
    r64, r32 = _step_oracle(c, torch.float64), _step_oracle(c, torch.float32)
    idx, report, ok = c["idx"], [], []
    for it in range(c["iters"]):
        for j, (key, hist) in enumerate((("wf", "wf_hist"), ("res", "res_hist"))):
            ok.append(_vs_float64(f"{hist}[{it}]", cv[hist][it][idx], r64[it][j], r32[it][j], report))
        for d, lv in enumerate(_levels(c["n"], c["depth"])):
            ok.append(_vs_float64(f"st_hist[{it}] level {d}", cv["st_hist"][it][idx][:, :, lv], r64[it][2][:, :, lv], r32[it][2][:, :, lv], report))
    last = c["iters"] - 1
    for key, hist in (("wf", "wf_hist"), ("res", "res_hist"), ("states", "st_hist")):      # the live buffers are the last slots
        assert torch.equal(cv[key], cv[hist][last]), key
    rmse = cv["res_hist"].double().pow(2).mean((2, 3, 4)).sqrt()
    assert float(((cv["rmse_hist"].double() - rmse).abs() / rmse).max()) <= 1e-5
    print(f"[{tag}] vs float64: " + "; ".join(report))
    assert all(ok), report


def _route_changes(c, which):
    """The last column of the DESIGN.md table, for the network calls: only the fp32 level-0 kernels of hn_dca.hip (W >= 256) have a twin with another
    summation order.  hn_cs.hip against the general kernel is bit-identical (the header's claim), so states_out / d_out / k_sq / src never change a bit."""
    dca = c["mode"] is None and c["n"] >= 256
    return dca and which in ("wf", "res", "states", "hist", "all", "states_in")


STEP_ROWS = ([("d4_256", w) for w in ("wf", "res", "states", "k_sq", "src", "hist", "all")] + [("d2_64", w) for w in ("states", "hist", "all")]
             + [("d4_272", w) for w in ("states", "all")] + [(t, "all") for t in ("d4_256_fp16", "d4_256_bf16x3", "d2_64_lanes2", "d2_64_graph")])


@pytest.mark.parametrize("tag,which", STEP_ROWS)
def test_step_on_offset_buffers(tag, which):
    c = _net_case(tag)
    eng = c["eng"]
    if "step_base" not in c:
        replays = eng.counter("graph_replays")
        c["step_base"], _ = _run_step(c, {})
        if tag == "d2_64_graph":
            assert eng.counter("graph_replays") - replays == c["iters"]        # the captured iteration, its buffers baked in, is what ran
        if c["mode"] is None:
            _step_vs_float64(tag + " aligned", c, c["step_base"])
    base = c["step_base"]
    runs = {}
    for k in KS:
        replays = eng.counter("graph_replays")
        runs[k], _ = _run_step(c, _step_offsets(which, k))
        if tag == "d2_64_graph":
            assert eng.counter("graph_replays") - replays == c["iters"]
        for name in ("k_sq", "src"):                                            # inputs stay inputs
            assert torch.equal(runs[k][name].cpu(), c["t"][name]), name
    _same_bits(f"{tag} {which} 2 vs 1", runs[2], runs[1], STEP_OUT, atomics=("rmse_hist",))
    _same_bits(f"{tag} {which} 3 vs 1", runs[3], runs[1], STEP_OUT, atomics=("rmse_hist",))
    _close_or_same(f"{tag} {which}", runs[1], base, STEP_OUT, _route_changes(c, which), atomics=("rmse_hist",))
    if c["mode"] is None:
        _step_vs_float64(f"{tag} {which}", c, runs[1])


@pytest.mark.parametrize("tag", ["d4_256", "d4_272", "d2_64", "d4_256_fp16"])
def test_step_routes_follow_the_alignment(tag):
    """What the profile names say (one iteration without histories, so that every kernel of the call sees the caller's buffers; with histories the
    later iterations read wf / res from the history slots and every second iteration reads the states from the library's buffer)."""
    c = _net_case(tag)
    dca = c["mode"] is None and c["n"] >= 256
    names = {w: _run_step(c, _step_offsets(w, 1), iters=1, hist=False, profile=True)[1] for w in ("aligned", "wf", "res", "states", "k_sq", "src", "all")}
    names["hist"] = _run_step(c, _step_offsets("hist", 1), profile=True)[1]
    print(f"[{tag}] " + "; ".join(f"{w}: {sorted(v)}" for w, v in names.items()))
    # where several levels share the merged launch of hn_cs.hip (accounted to conv_state0) its standing down shows as one name per level
    split = "conv_state0" in names["aligned"] and "conv_state1" not in names["aligned"] and c["n"] >= 256
    for w, got in names.items():
        if split:
            assert ("conv_state1" in got) == (w in ("states", "all")), (w, sorted(got))
        if not dca:                                  # no other route looks at the alignment here
            assert {x for x in got if not x.startswith("conv_state")} == {x for x in names["aligned"] if not x.startswith("conv_state")}, w
            continue
        if w in ("aligned", "k_sq", "src"):
            assert "inc_conv_signal0" in got and not ({"inc", "conv_signal0"} & got), (w, sorted(got))
        elif w == "hist":                            # iteration 0 reads the aligned wf / res: paired; iterations 1, 2 read the misaligned slots
            assert {"inc_conv_signal0", "inc", "conv_signal0"} <= got, (w, sorted(got))
        else:
            assert {"inc", "conv_signal0"} <= got and "inc_conv_signal0" not in got, (w, sorted(got))
        if tag == "d4_256":
            assert "deep" in got, w                  # k_deepx reads and writes the states with plain 16- / 8-byte accesses: no alignment route


def _run_unet(c, offsets):
    eng = c["eng"]
    cv = Carved(c["u"], DEV, offsets)
    rc = eng.lib.hn_unet(eng.ctx, _ptr(cv["in6"]), _ptr(cv["states_in"]), _ptr(cv["states_out"]), _ptr(cv["d_out"]), c["b"], eng._stream())
    assert rc == 0, eng.lib.hn_last_error(eng.ctx)
    _done(eng, cv)
    return cv


def _unet_oracle(c, dtype):
    key = ("unet_oracle", dtype)
    if key not in c:
        w = {k: torch.from_numpy(v).to(dtype) for k, v in c["w"].items()}
        st = O.unflatten_states(c["u"]["states_in"][c["idx"]].to(dtype), c["n"], c["depth"])
        d, new = O.unet_forward(c["u"]["in6"][c["idx"]].to(dtype), st, w, c["depth"], "prelu")
        c[key] = (d, O.flatten_states(new))
    return c[key]


def _unet_vs_float64(tag, c, cv):
    (d64, s64), (d32, s32) = _unet_oracle(c, torch.float64), _unet_oracle(c, torch.float32)
    idx = c["idx"]
    if c["mode"] is not None:        # the 16-bit modes: their bars of tests/test_config_matrix.py / tests/test_gpu_parity.py on d
        scale = float(d64.abs().max())
        err = float((cv["d_out"][idx].cpu().double() - d64).abs().max()) / scale
        ora = float((d32.double() - d64).abs().max()) / scale
        print(f"[{tag}] d vs float64: {err:.2e} (fp32 oracle {ora:.2e})")
        assert err <= (5e-3 if c["mode"] == "fp16" else min(1e-5, 1.25 * ora)), (err, ora)
        return
    report = []
    ok = [_vs_float64("d", cv["d_out"][idx], d64, d32, report)]
    for lv_i, lv in enumerate(_levels(c["n"], c["depth"])):
        ok.append(_vs_float64(f"state{lv_i}", cv["states_out"][idx][:, :, lv], s64[:, :, lv], s32[:, :, lv], report))
    print(f"[{tag}] vs float64: " + "; ".join(report))
    assert all(ok), report


UNET_ROWS = ([("d4_256", w) for w in ("in6", "states_in", "states_out", "d_out", "all")] + [("d2_64", w) for w in ("states_in", "states_out", "all")]
             + [(t, "all") for t in ("d4_272", "d4_256_fp16", "d4_256_bf16x3")])


@pytest.mark.parametrize("tag,which", UNET_ROWS)
def test_unet_on_offset_buffers(tag, which):
    c = _net_case(tag)
    if "unet_base" not in c:
        c["unet_base"] = _run_unet(c, {})
        _unet_vs_float64(tag + " aligned", c, c["unet_base"])
    runs = {k: _run_unet(c, {name: k for name in c["u"]} if which == "all" else {which: k}) for k in KS}
    out = ("d_out", "states_out")
    for k in KS:
        assert torch.equal(runs[k]["in6"].cpu(), c["u"]["in6"]) and torch.equal(runs[k]["states_in"].cpu(), c["u"]["states_in"])
    _same_bits(f"{tag} {which} 2 vs 1", runs[2], runs[1], out)
    _same_bits(f"{tag} {which} 3 vs 1", runs[3], runs[1], out)
    _close_or_same(f"{tag} unet {which}", runs[1], c["unet_base"], out, _route_changes(c, "states_in" if which == "all" else which))
    _unet_vs_float64(f"{tag} {which}", c, runs[1])


# =====================================================================================================================================
# 1b. the spectral operator: one size per route
# =====================================================================================================================================
# (n, options, hn_get_counter(HN_CNT_SPECTRAL_ROUTE)): 1 power of two, 2 prime-factor, 3 dense, 4 mixed
SPEC_CASES = ([(32, {}, 1), (48, {}, 2), (96, {"spectral_pfa": 0}, 3), (144, {"spectral_mixed": 1}, 4)]
              + [(256, {"spectral_radix16": r, "spectral_cols": cc}, 1) for r in (0, 1, 2) for cc in (0, 1, 2)])
SPEC_IDS = [f"{n}" + "".join(f"-{k.replace('spectral_', '')}{v}" for k, v in o.items()) for n, o, _ in SPEC_CASES]
SPEC_B = 2
_spec_engines = {}


@pytest.fixture(scope="module")
def spec_engines():
    yield _spec_engines
    for e in _spec_engines.values():
        e.close()
    _spec_engines.clear()


def _spec_engine(cache, case):
    from helmnet_amd.engine import Engine
    n, options, route = case
    key = (n, tuple(sorted(options.items())))
    if key not in cache:
        e = Engine(DEV)
        for k, v in options.items():
            e.set_option(k, v)
        e.set_domain(n, *SP.DOMAIN)
        assert e.counter("spectral_route") == route
        cache[key] = e
    return cache[key]


def _spec_runs(eng, tensors, call):
    """``call(cv)`` on plain tensors and at offsets 1, 2, 3 (every tensor of the call offset) -> {0: plain, 1: ..., 2: ..., 3: ...}."""
    runs = {}
    for k in (0,) + KS:
        cv = Carved(tensors, DEV, {name: k for name in tensors} if k else {})
        rc = call(cv)
        assert rc == 0, eng.lib.hn_last_error(eng.ctx)
        _done(eng, cv)
        runs[k] = cv
    return runs


def _spec_check(tag, runs, out, want, bar, inputs):
    for k in KS:
        _same_bits(f"{tag} offset {k}", runs[k], runs[0], (out,))
        for name in inputs:
            assert torch.equal(runs[k][name], runs[0][name]), name
    ratio = SP.errors(runs[1][out], want) / bar
    print(f"[{tag}] error / (scale * max|u|): " + ", ".join(f"{float(r) * SP.BAR:.2e}" for r in ratio) + f" (bar {SP.BAR:.0e})")
    assert float(ratio.max()) <= 1.0, (tag, ratio)


@pytest.mark.parametrize("case", SPEC_CASES, ids=SPEC_IDS)
def test_laplacian_on_offset_buffers(spec_engines, case):
    eng, n = _spec_engine(spec_engines, case), case[0]
    c = SP.forward_case(n)
    t = {"wf": c["u"][:SPEC_B], "out": torch.full((SPEC_B, 2, n, n), NAN)}
    runs = _spec_runs(eng, t, lambda cv: eng.lib.hn_laplacian(eng.ctx, _ptr(cv["wf"]), _ptr(cv["out"]), SPEC_B, eng._stream()))
    _spec_check(f"laplacian {n}", runs, "out", c["lap"][:SPEC_B], c["bar_lap"][:SPEC_B], ("wf",))


@pytest.mark.parametrize("src_batch", [1, SPEC_B])
@pytest.mark.parametrize("case", SPEC_CASES, ids=SPEC_IDS)
def test_residual_on_offset_buffers(spec_engines, case, src_batch):
    eng, n = _spec_engine(spec_engines, case), case[0]
    c = SP.forward_case(n)
    one = src_batch == 1
    t = {"wf": c["u"][:SPEC_B], "k_sq": c["k_sq"][:SPEC_B], "src": c["src1"] if one else c["src2"], "res": torch.full((SPEC_B, 2, n, n), NAN)}
    runs = _spec_runs(eng, t, lambda cv: eng.lib.hn_residual(eng.ctx, _ptr(cv["wf"]), _ptr(cv["k_sq"]), _ptr(cv["src"]), src_batch, _ptr(cv["res"]),
                                                             SPEC_B, eng._stream()))
    _spec_check(f"residual {n} src_batch {src_batch}", runs, "res", (c["res1"] if one else c["res2"])[:SPEC_B],
                (c["bar_res1"] if one else c["bar_res2"])[:SPEC_B], ("wf", "k_sq", "src"))


@pytest.mark.parametrize("case", SPEC_CASES, ids=SPEC_IDS)
def test_residual_vjp_on_offset_buffers(spec_engines, case):
    eng, n = _spec_engine(spec_engines, case), case[0]
    c = SP.adjoint_case(n)
    t = {"g": c["g"][:SPEC_B], "k_sq": c["k_sq"][:SPEC_B], "out": torch.full((SPEC_B, 2, n, n), NAN)}
    runs = _spec_runs(eng, t, lambda cv: eng.lib.hn_residual_vjp(eng.ctx, _ptr(cv["g"]), _ptr(cv["k_sq"]), _ptr(cv["out"]), SPEC_B, eng._stream()))
    _spec_check(f"residual_vjp {n}", runs, "out", c["vjp"][:SPEC_B], c["bar"][:SPEC_B], ("g", "k_sq"))


@pytest.mark.parametrize("n", [32, 48, 256])
def test_rmse_on_offset_buffers(spec_engines, n):
    """hn_rmse: one kernel whatever the alignment; its per-sample sums are float atomics, so two runs agree to rounding, not bit for bit (rtol 1e-5,
    the suite's bar for such sums)."""
    eng = _spec_engine(spec_engines, (n, {}, 1 if n != 48 else 2))
    c = SP.forward_case(n)
    res = c["res1"][:SPEC_B].float()
    t = {"res": res, "rmse": torch.full((SPEC_B,), NAN)}
    runs = _spec_runs(eng, t, lambda cv: eng.lib.hn_rmse(eng.ctx, _ptr(cv["res"]), _ptr(cv["rmse"]), SPEC_B, eng._stream()))
    want = res.double().pow(2).mean((1, 2, 3)).sqrt()
    for k in (0,) + KS:
        assert torch.equal(runs[k]["res"].cpu(), res)
        assert torch.allclose(runs[k]["rmse"], runs[0]["rmse"], rtol=1e-5, atol=0)
        assert float(((runs[k]["rmse"].cpu().double() - want).abs() / want).max()) <= 1e-5, k


# =====================================================================================================================================
# 1c. the sub-module calls at 32 x 48
# =====================================================================================================================================
MOD_H, MOD_W, MOD_B = 32, 48, 2


@pytest.fixture(scope="module")
def mod_engine():
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    yield e
    e.close()


def _module_check(tag, eng, x, out_shape, call, ref):
    t = {"x": x, "out": torch.full(out_shape, NAN)}
    runs = _spec_runs(eng, t, call)
    for k in KS:
        _same_bits(f"{tag} offset {k}", runs[k], runs[0], ("out",))
        assert torch.equal(runs[k]["x"].cpu(), x)
    report = []
    ok = _vs_float64(tag, runs[1]["out"], ref(torch.float64), ref(torch.float32), report)
    print(f"[{tag}] vs float64: {report[0]}")
    assert ok, report


@pytest.mark.parametrize("cin,cout", [(6, 8), (8, 8), (10, 8), (16, 8), (10, 2)])
def test_double_conv_on_offset_buffers(mod_engine, cin, cout):
    eng = mod_engine
    g = torch.Generator().manual_seed(100 * cin + cout)
    x = torch.randn(MOD_B, cin, MOD_H, MOD_W, generator=g)
    w = {"m.double_conv.0.weight": torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5), "m.double_conv.0.bias": 0.05 * torch.randn(cout, generator=g),
         "m.double_conv.1.weight": torch.tensor([-0.4]), "m.double_conv.2.weight": torch.randn(cout, cout, 3, 3, generator=g) / (3.0 * cout ** 0.5),
         "m.double_conv.2.bias": 0.05 * torch.randn(cout, generator=g)}
    blob = eng._host_blob(list(w.values()))
    bp = blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    _module_check(f"double_conv {cin}->{cout}", eng, x, (MOD_B, cout, MOD_H, MOD_W),
                  lambda cv: eng.lib.hn_double_conv(eng.ctx, _ptr(cv["x"]), cin, cout, bp, 0, _ptr(cv["out"]), MOD_B, MOD_H, MOD_W, eng._stream()),
                  lambda dt: O.double_conv(x.to(dt), {k: v.to(dt) for k, v in w.items()}, "m"))


@pytest.mark.parametrize("transposed", [0, 1])
def test_conv8x8_on_offset_buffers(mod_engine, transposed):
    eng = mod_engine
    g = torch.Generator().manual_seed(88 + transposed)
    x = torch.randn(MOD_B, 8, MOD_H, MOD_W, generator=g)
    w, bias = torch.randn(8, 8, 8, 8, generator=g) / 16.0, 0.05 * torch.randn(8, generator=g)
    blob = eng._host_blob([w, bias])
    bp = blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    shape = (MOD_B, 8, 2 * MOD_H, 2 * MOD_W) if transposed else (MOD_B, 8, MOD_H // 2, MOD_W // 2)
    conv = F.conv_transpose2d if transposed else F.conv2d
    _module_check(f"conv8x8 transposed={transposed}", eng, x, shape,
                  lambda cv: eng.lib.hn_conv8x8(eng.ctx, _ptr(cv["x"]), bp, transposed, _ptr(cv["out"]), MOD_B, MOD_H, MOD_W, eng._stream()),
                  lambda dt: conv(x.to(dt), w.to(dt), bias.to(dt), stride=2, padding=3))


def test_out_conv_on_offset_buffers(mod_engine):
    eng = mod_engine
    g = torch.Generator().manual_seed(82)
    x = torch.randn(MOD_B, 8, MOD_H, MOD_W, generator=g)
    w, bias = torch.randn(2, 8, 1, 1, generator=g) / 3.0, 0.05 * torch.randn(2, generator=g)
    blob = eng._host_blob([w, bias])
    bp = blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    _module_check("out_conv", eng, x, (MOD_B, 2, MOD_H, MOD_W),
                  lambda cv: eng.lib.hn_out_conv(eng.ctx, _ptr(cv["x"]), bp, _ptr(cv["out"]), MOD_B, MOD_H, MOD_W, eng._stream()),
                  lambda dt: F.conv2d(x.to(dt), w.to(dt), bias.to(dt)))


# =====================================================================================================================================
# 1d. the float64 family at n = 48, batch 2, on doubles 8 bytes past a 16-byte boundary
# =====================================================================================================================================
F64_N, F64_B = 48, 2


@pytest.fixture(scope="module")
def eng64(weights):
    from test_f64_solver_gpu import _engine
    e = _engine(weights)
    e.set_domain(F64_N, 8, 2.0, 1.0)
    yield e
    e.close()


def _f64_runs(eng, tensors, call):
    runs = {}
    for k in (0, 1):
        cv = Carved(tensors, DEV, {name: 1 for name in tensors} if k else {})
        rc = call(cv)
        assert rc == 0, eng.lib.hn_last_error(eng.ctx)
        _done(eng, cv)
        runs[k] = cv
        assert all(v is None or v.data_ptr() % 16 == 8 * k for v in cv.t.values())
    return runs


def _rel(got, want):
    return float((got.cpu() - want).abs().max()) / float(want.abs().max())


def test_laplacian_and_residual_f64_on_offset_buffers(eng64):
    """The float64 operator sums in a fixed order: the offset call gives the bits of the plain one, and both meet the bar of tests/test_f64_gpu.py."""
    from test_f64_gpu import BAR, case
    c = case(F64_N, F64_B, 1)
    eng = eng64
    t = {"wf": c["wf"], "k_sq": c["k_sq"], "src": c["src"], "lap": torch.full_like(c["wf"], NAN), "res": torch.full_like(c["wf"], NAN),
         "rmse": torch.full((F64_B,), NAN, dtype=torch.float64)}

    def call(cv):
        rc = eng.lib.hn_laplacian_f64(eng.ctx, _ptr(cv["wf"]), _ptr(cv["lap"]), F64_B, eng._stream())
        return rc or eng.lib.hn_residual_f64(eng.ctx, _ptr(cv["wf"]), _ptr(cv["k_sq"]), _ptr(cv["src"]), 1, _ptr(cv["res"]), _ptr(cv["rmse"]), F64_B, eng._stream())

    runs = _f64_runs(eng, t, call)
    _same_bits("f64 operator", runs[1], runs[0], ("lap", "res", "rmse", "wf", "k_sq", "src"))
    e_lap, e_res = _rel(runs[1]["lap"], c["lap"]), _rel(runs[1]["res"], c["res"])
    want = c["res"].pow(2).mean((1, 2, 3)).sqrt()
    e_rmse = float(((runs[1]["rmse"].cpu() - want).abs() / want).max())
    print(f"[f64 operator, offset 1 double] laplacian {e_lap:.2e}, residual {e_res:.2e}, rmse {e_rmse:.2e} (bar {BAR:.0e})")
    assert max(e_lap, e_res, e_rmse) <= BAR


def test_unet_f64_on_offset_buffers(eng64, weights):
    from test_f64_solver_gpu import BAR_UNET, DEPTH, unet_case
    c = unet_case(weights, F64_N, F64_B)
    eng = eng64
    t = {"in6": c["x"], "states_in": c["st"], "states_out": torch.full_like(c["st"], NAN), "d_out": torch.full((F64_B, 2, F64_N, F64_N), NAN, dtype=torch.float64)}
    runs = _f64_runs(eng, t, lambda cv: eng.lib.hn_unet_f64(eng.ctx, _ptr(cv["in6"]), _ptr(cv["states_in"]), _ptr(cv["states_out"]), _ptr(cv["d_out"]),
                                                              F64_B, eng._stream()))
    _same_bits("hn_unet_f64", runs[1], runs[0], ("d_out", "states_out", "in6", "states_in"))
    errs = [_rel(runs[1]["d_out"], c["d"])] + [_rel(a, b) for a, b in zip(O.unflatten_states(runs[1]["states_out"], F64_N, DEPTH), c["new"])]
    print(f"[hn_unet_f64, offset 1 double] d and the new states by level: {['%.2e' % v for v in errs]} (bar {BAR_UNET:.0e})")
    assert max(errs) <= BAR_UNET


def test_step_f64_on_offset_buffers(eng64, weights):
    from test_f64_solver_gpu import BAR_STEP, step_case
    c = step_case(weights, F64_N, F64_B, 1)
    eng, iters = eng64, 3
    L = c["st0"].shape[-1]
    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64)  # noqa: E731
    t = {"wf": c["wf0"], "res": c["res0"], "states": c["st0"], "k_sq": c["k_sq"], "src": c["src"], "res_hist": new(iters, F64_B, 2, F64_N, F64_N),
         "wf_hist": new(iters, F64_B, 2, F64_N, F64_N), "st_hist": new(iters, F64_B, 2, L), "rmse_hist": new(iters, F64_B)}
    runs = _f64_runs(eng, t, lambda cv: eng.lib.hn_step_f64(eng.ctx, *[_ptr(cv[k]) for k in LIVE], 1, F64_B, iters, *[_ptr(cv[h]) for h in HIST], eng._stream()))
    _same_bits("hn_step_f64", runs[1], runs[0], STEP_OUT + ("k_sq", "src"))
    errs = {}
    for it in range(iters):
        errs[f"wf_hist[{it}]"] = _rel(runs[1]["wf_hist"][it], c["wf"][it])
        errs[f"res_hist[{it}]"] = _rel(runs[1]["res_hist"][it], c["res"][it])
        errs[f"st_hist[{it}]"] = _rel(runs[1]["st_hist"][it], c["st"][it])
        errs[f"rmse_hist[{it}]"] = float(((runs[1]["rmse_hist"][it].cpu() - c["rmse"][it]).abs() / c["rmse"][it]).max())
    for key, hist in (("wf", "wf_hist"), ("res", "res_hist"), ("states", "st_hist")):
        assert torch.equal(runs[1][key], runs[1][hist][-1]), key
    worst = max(errs, key=errs.get)
    print(f"[hn_step_f64, offset 1 double] worst {worst} {errs[worst]:.2e} (bar {BAR_STEP:.0e})")
    assert errs[worst] <= BAR_STEP, errs


# =====================================================================================================================================
# 2. training calls: no kernel of hn_train.hip looks at the alignment, so every output keeps its bits
# =====================================================================================================================================
TRAIN_IN = ("weights", "wf", "res", "states", "k_sq", "src")
TRAIN_OUT = ("wf_hist", "res_hist", "st_hist", "loss", "grad", "grad_wf0", "grad_res0", "grad_st0")
VJP_COT = ("g_wf_hist", "g_res_hist", "g_st_hist")
VJP_OUT = ("g_wf0", "g_res0", "g_st0", "g_k_sq", "g_src", "g_weights")


@pytest.fixture(scope="module")
def train_solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.to(DEV)
    return s


@pytest.mark.parametrize("n", [32, 96])
def test_train_grad_and_step_vjp_on_offset_buffers(train_solver, weights, n):
    """hn_train_grad (two unrolled iterations) and hn_step_vjp over the histories it wrote, every tensor of both calls one float past a 16-byte
    boundary: the bits of the plain calls, and the gradients against float64 autograd of the oracle on the bars of tests/train_matrix.py.  32^2: every
    level on the default fused launches; 96^2: level 0 on the tiled backward launch."""
    from helmnet_amd.engine import pack_weights
    b, T = 2, 2
    train_solver.set_domain_size(n, source_location=[n // 3, n // 2])
    eng = train_solver.engine()
    ti = teacher_inputs(n, b, seed=1200 + n)
    wf, res, st, sos = (torch.from_numpy(ti[k]) for k in ("wf", "res", "states", "sos"))
    case = TM.make_case(4, "prelu", 4, n, b, {k: v.detach() for k, v in weights.items()}, wf, res, 0.2 * st, sos)
    L, n_w = case["L"], int(eng.lib.hn_weight_count(8, 4, 2))
    cot = TM.cotangents(T, b, n, L, 1300 + n)
    new = lambda *shape: torch.full(shape, NAN)  # noqa: E731
    t = {"weights": torch.from_numpy(pack_weights(case["w"], 4, "prelu", 4)), "wf": case["wf"], "res": case["res"], "states": case["st"], "k_sq": case["k_sq"],
         "src": case["src"].contiguous(), "wf_hist": new(T, b, 2, n, n), "res_hist": new(T, b, 2, n, n), "st_hist": new(T, b, 2, L), "loss": new(1),
         "grad": new(n_w), "grad_wf0": new(b, 2, n, n), "grad_res0": new(b, 2, n, n), "grad_st0": new(b, 2, L),
         "g_wf_hist": cot["wf"], "g_res_hist": cot["res"], "g_st_hist": cot["st"], "g_wf0": new(b, 2, n, n), "g_res0": new(b, 2, n, n), "g_st0": new(b, 2, L),
         "g_k_sq": torch.zeros(b, 1, n, n), "g_src": torch.zeros(1, 2, n, n), "g_weights": torch.zeros(n_w)}
    assert t["weights"].numel() == n_w
    runs = {}
    for k in (0, 1):
        cv = Carved(t, DEV, {name: 1 for name in t} if k else {})
        rc = eng.lib.hn_train_grad(eng.ctx, *[_ptr(cv[x]) for x in TRAIN_IN], 1, b, T, 1e4, *[_ptr(cv[x]) for x in TRAIN_OUT], eng._stream())
        assert rc == 0, eng.lib.hn_last_error(eng.ctx)
        _done(eng, cv)
        rc = eng.lib.hn_step_vjp(eng.ctx, _ptr(cv["weights"]), _ptr(cv["wf"]), _ptr(cv["res"]), _ptr(cv["states"]), _ptr(cv["k_sq"]), 1, b, T,
                                 _ptr(cv["wf_hist"]), _ptr(cv["res_hist"]), _ptr(cv["st_hist"]), *[_ptr(cv[x]) for x in VJP_COT], None, None, None,
                                 *[_ptr(cv[x]) for x in VJP_OUT], 0, eng._stream())
        assert rc == 0, eng.lib.hn_last_error(eng.ctx)
        _done(eng, cv)
        runs[k] = cv
    same = tuple(x for x in TRAIN_IN + TRAIN_OUT + VJP_COT + VJP_OUT if x != "loss")
    _same_bits(f"training {n}", runs[1], runs[0], same)
    assert torch.allclose(runs[1]["loss"], runs[0]["loss"], rtol=1e-6, atol=0)      # (the loss is a sum of float atomics)
    # the oracle: one float64 graph, both legs; the fp32 oracle's own distance sets the bar where it is above half the base bar (TM.bars)
    cv = runs[1]
    got = {"fwd": {"wf1": cv["wf_hist"][0].cpu(), "res1": cv["res_hist"][0].cpu(), "st1": cv["st_hist"][0].cpu()}, "loss": float(cv["loss"][0]),
           "a": {"in": {"wf": cv["grad_wf0"].cpu(), "res": cv["grad_res0"].cpu(), "st": cv["grad_st0"].cpu()}, "w": TM._named_grads(case, cv["grad"]), "tape": {}},
           "b": {"in": {"wf": cv["g_wf0"].cpu(), "res": cv["g_res0"].cpu(), "st": cv["g_st0"].cpu(), "k_sq": cv["g_k_sq"].cpu(), "src": cv["g_src"].cpu()},
                 "w": TM._named_grads(case, cv["g_weights"]), "tape": {}}}
    want = TM.oracle_legs(case, torch.float64, None, cot, n_unroll=T)
    fwd, ea, eb = TM.compare(case, got, want, whole_tape=False)
    _, oa, ob = TM.compare(case, TM.oracle_legs(case, torch.float32, None, cot, n_unroll=T), want, strict=False, whole_tape=False)
    TM.report(fwd, TM.FWD_BAR)
    assert abs(got["loss"] - want["loss"]) <= 1e-5 * want["loss"]
    TM.assert_bars(f"offset training {n}", {"a": (ea, TM.bars(oa)), "b": (eb, TM.bars(ob)), "fwd": fwd})


def test_adam_step_on_offset_buffers(train_solver):
    """n = 1001 on weights / grad / both moments one float and the mask one byte past a 16-byte boundary: the bits of the plain call, and torch's Adam."""
    eng = train_solver.engine()
    n = 1001
    g = torch.Generator().manual_seed(1001)
    mask = (torch.rand(n, generator=g) > 0.2).to(torch.uint8)
    t = {"weights": torch.randn(n, generator=g), "grad": torch.randn(n, generator=g), "exp_avg": 0.1 * torch.randn(n, generator=g),
         "exp_avg_sq": 0.1 * torch.rand(n, generator=g)}
    runs = {}
    for k in (0, 1):
        cv = Carved(t, DEV, {name: 1 for name in t} if k else {})
        m = torch.empty(n + 16 + k, dtype=torch.uint8, device=DEV)
        start = (-m.data_ptr()) % 16 + k
        mv = m[start:start + n]
        mv.copy_(mask)
        assert mv.data_ptr() % 16 == k
        rc = eng.lib.hn_adam_step(eng.ctx, _ptr(cv["weights"]), _ptr(cv["grad"]), _ptr(cv["exp_avg"]), _ptr(cv["exp_avg_sq"]), _ptr(mv), n, 1e-3, 0.9, 0.95, 1e-8,
                                  1e-2, 0.5, 3, eng._stream())
        assert rc == 0, eng.lib.hn_last_error(eng.ctx)
        _done(eng, cv)
        assert torch.equal(mv.cpu(), mask)
        runs[k] = cv
    _same_bits("adam", runs[1], runs[0], tuple(t))
    keep = mask.bool()
    assert torch.equal(runs[1]["weights"].cpu()[~keep], t["weights"][~keep]) and torch.equal(runs[1]["exp_avg"].cpu()[~keep], t["exp_avg"][~keep])
    # one step of torch's Adam from the same moments: g = clip(grad) + wd * p, step 3
    p, gr = t["weights"].double(), t["grad"].double().clamp(-0.5, 0.5)
    gr = gr + 1e-2 * p
    m1, v1 = 0.9 * t["exp_avg"].double() + 0.1 * gr, 0.95 * t["exp_avg_sq"].double() + 0.05 * gr * gr
    want = p - 1e-3 / (1 - 0.9 ** 3) * m1 / (v1.sqrt() / (1 - 0.95 ** 3) ** 0.5 + 1e-8)
    assert float((runs[1]["weights"].cpu().double() - want)[keep].abs().max()) <= 2e-6      # the bar of tests/test_training_gpu.py for one kernel step


# =====================================================================================================================================
# 3. histories that overlap the live buffers, and hn_unet's states
# =====================================================================================================================================
OVERLAP_K = 4
FORMS = {"zero_copy": ({}, 2), "hist_copy": ({"hist_copy": 1}, 2), "lanes2": ({"lanes": 2}, 4), "graph": ({"graph": 1}, 2)}
_overlap = {}


def _overlap_case(b):
    """d2_64 at 64^2: inputs, the solver and the results of the call on separate buffers (K = 4, all four histories)."""
    if b not in _overlap:
        n, depth, K = 64, 2, OVERLAP_K
        w = config_weights(depth, 744, "B", n=n)
        s = _solver(depth, "prelu", depth, w, n)
        eng = s.engine()
        x = config_input(n, b, depth, 9500 + b, wf_scale=1e-6)
        g = torch.Generator().manual_seed(9600 + b)
        t = {"wf": torch.from_numpy(x["wf"]), "res": torch.from_numpy(x["res"]), "states": torch.from_numpy(x["states"]),
             "k_sq": (1.0 / torch.from_numpy(x["sos"])) ** 2, "src": 1e-3 * torch.randn(1, 2, n, n, generator=g)}
        d = {k: v.to(DEV).contiguous() for k, v in t.items()}
        d.update(res_hist=torch.full((K, b, 2, n, n), NAN, device=DEV), wf_hist=torch.full((K, b, 2, n, n), NAN, device=DEV),
                 st_hist=torch.full((K, b, 2, eng.state_len), NAN, device=DEV), rmse_hist=torch.full((K, b), NAN, device=DEV))
        eng.step(*[d[k] for k in LIVE], K, *[d[h] for h in HIST])
        torch.cuda.synchronize()
        eng.check_async_errors()
        _overlap[b] = dict(n=n, b=b, s=s, eng=eng, t=t, ref=d)
    return _overlap[b]


def _overlapping_call(c, live, slot, shift):
    """hn_step with ``live`` (wf or res) a view of its own history: ``slot`` slots and ``shift`` floats into it.  -> (status, message, the tensors)."""
    eng, n, b, K = c["eng"], c["n"], c["b"], OVERLAP_K
    per = b * 2 * n * n
    d = {k: v.to(DEV).contiguous() for k, v in c["t"].items()}
    flat = torch.full(((K + 1) * per,), NAN, device=DEV)          # one slot more than the history: a shifted view of the last slot stays inside
    hist = live + "_hist"
    d[hist] = flat[:K * per].view(K, b, 2, n, n)
    start = slot * per + shift
    view = flat[start:start + per].view(b, 2, n, n)
    view.copy_(d[live])
    d[live] = view
    other = "wf_hist" if live == "res" else "res_hist"
    d[other] = torch.full((K, b, 2, n, n), NAN, device=DEV)
    d["st_hist"] = torch.full((K, b, 2, eng.state_len), NAN, device=DEV)
    d["rmse_hist"] = torch.full((K, b), NAN, device=DEV)
    before = {k: v.clone() for k, v in d.items()}
    before["flat"] = flat.clone()
    d["flat"] = flat
    its = eng.counter("eager_iterations") + eng.counter("graph_replays")
    rc = eng.lib.hn_step(eng.ctx, *[_ptr(d[k]) for k in LIVE], 1, b, K, *[_ptr(d[h]) for h in HIST], eng._stream())
    msg = eng.lib.hn_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    eng.check_async_errors()
    ran = eng.counter("eager_iterations") + eng.counter("graph_replays") - its
    return rc, msg, d, before, ran


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("live", ["res", "wf"])
def test_a_live_buffer_inside_its_history_is_refused_except_as_slot_0(live, form):
    """The contract of include/helmnet_hip.h (hn_step): a live buffer that overlaps its history anywhere but exactly at slot 0 is refused with
    HN_ERR_ARG naming both arguments and nothing is enqueued -- slot 1 (which the zero-copy form used to overwrite with the final residual without a
    word), the last slot, and a view shifted by one plane; equal pointers run the copying form as before: rows 1 .. K - 1, the live buffers and the
    states are the bits of the call on separate buffers, and row 0, being the live buffer, holds the final value.  In every form of the loop."""
    options, b = FORMS[form]
    c = _overlap_case(b)
    eng, n, K, ref = c["eng"], c["n"], OVERLAP_K, c["ref"]
    for k, v in options.items():
        eng.set_option(k, v)
    try:
        hist = live + "_hist"
        for slot, shift in ((1, 0), (K - 1, 0), (1, n * n), (0, n * n), (0, 1)):
            rc, msg, d, before, ran = _overlapping_call(c, live, slot, shift)
            assert rc == -1 and f"{live} overlaps {hist}" in msg, (slot, shift, rc, msg)
            assert ran == 0, (slot, shift)
            for k, v in before.items():          # nothing was enqueued: every buffer holds what it held (NaN compares by bits)
                assert torch.equal(d[k].view(torch.int32), v.view(torch.int32)), (slot, shift, k)
        rc, msg, d, _, ran = _overlapping_call(c, live, 0, 0)
        assert rc == 0, msg
        assert ran == K
        assert d[live].data_ptr() == d[hist].data_ptr()
        for k in ("wf", "res", "states", "st_hist", "wf_hist" if live == "res" else "res_hist"):
            assert torch.equal(d[k], ref[k]), k
        assert torch.equal(d[hist][1:], ref[hist][1:]) and torch.equal(d[hist][0], ref[live])
        assert torch.allclose(d["rmse_hist"], ref["rmse_hist"], rtol=1e-5, atol=0)
    finally:
        for k in options:
            eng.set_option(k, 1 if k == "lanes" else 0)


def test_other_overlaps_of_step_arguments_are_refused_too():
    """wf against the residual history, the state history against the states, two histories in one buffer: refused by name; two inputs that are
    only read may share memory."""
    c = _overlap_case(2)
    eng, n, b, K = c["eng"], c["n"], 2, OVERLAP_K
    d = {k: v.to(DEV).contiguous() for k, v in c["t"].items()}
    hist = torch.full((K, b, 2, n, n), NAN, device=DEV)
    st_hist = torch.full((K, b, 2, eng.state_len), NAN, device=DEV)

    def call(**kw):
        a = dict(d, res_hist=None, wf_hist=None, st_hist=None, rmse_hist=None)
        a.update(kw)
        rc = eng.lib.hn_step(eng.ctx, *[_ptr(a[k]) for k in LIVE], 1, b, K, *[_ptr(a[h]) for h in HIST], eng._stream())
        return rc, eng.lib.hn_last_error(eng.ctx).decode()

    its = eng.counter("eager_iterations")
    for kw, text in ((dict(res_hist=hist, wf=hist[1]), "wf overlaps res_hist"), (dict(st_hist=st_hist, states=st_hist[2]), "states overlaps st_hist"),
                     (dict(res_hist=hist, wf_hist=hist), "res_hist overlaps wf_hist"), (dict(res=d["wf"]), "wf overlaps res"),
                     (dict(wf_hist=hist, rmse_hist=hist.view(-1)[8:8 + K * b].view(K, b)), "wf_hist overlaps rmse_hist"),
                     (dict(k_sq=d["wf"].view(-1)[: b * n * n].view(b, 1, n, n)), "wf overlaps k_sq")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (text, rc, msg)
    assert eng.counter("eager_iterations") == its
    src2 = d["k_sq"].view(-1)[: 2 * n * n].view(1, 2, n, n)          # read against read
    rc, msg = call(src=src2)
    torch.cuda.synchronize()
    assert rc == 0, msg


def test_unet_refuses_states_that_overlap():
    """hn_unet writes states_out level by level while later kernels still read states_in: equal pointers (the documented rule) and a partial overlap
    (not refused before) both return HN_ERR_ARG naming the two, and nothing is written."""
    c = _overlap_case(2)
    eng, n, b = c["eng"], c["n"], 2
    L = eng.state_len
    x6 = torch.from_numpy(config_input(n, b, 2, 9700, wf_scale=1e-6)["x6"]).to(DEV)
    flat = torch.full((2 * b * 2 * L,), 0.25, device=DEV)
    st_in = flat[: b * 2 * L].view(b, 2, L)
    d_out = torch.full((b, 2, n, n), NAN, device=DEV)
    for shift in (0, n * n, b * 2 * L - 1):
        st_out = flat[shift:shift + b * 2 * L].view(b, 2, L)
        rc = eng.lib.hn_unet(eng.ctx, _ptr(x6), _ptr(st_in), _ptr(st_out), _ptr(d_out), b, eng._stream())
        msg = eng.lib.hn_last_error(eng.ctx).decode()      # (equal pointers are caught first, by the older check with its own wording)
        assert rc == -1 and ("states_in must not alias states_out" if shift == 0 else "states_in overlaps states_out") in msg, (shift, msg)
    rc = eng.lib.hn_unet(eng.ctx, _ptr(x6), _ptr(st_in), _ptr(flat[b * 2 * L:].view(b, 2, L)), _ptr(x6.view(-1)[: b * 2 * n * n].view(b, 2, n, n)), b, eng._stream())
    assert rc == -1 and "in6 overlaps d_out" in eng.lib.hn_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_out).all()) and bool((flat == 0.25).all())
    rc = eng.lib.hn_unet(eng.ctx, _ptr(x6), _ptr(st_in), _ptr(flat[b * 2 * L:].view(b, 2, L)), _ptr(d_out), b, eng._stream())      # adjacent, not overlapping
    torch.cuda.synchronize()
    eng.check_async_errors()
    assert rc == 0 and bool(torch.isfinite(d_out).all()) and bool((st_in == 0.25).all())
