"""Rectangular H x W domains (hn_set_domain_rect) through the C ABI against the float64 CPU oracle.  Needs a real MI355X.

Reference: the oracle on the per-axis tables of tests/rect_common.py (pinned by tests/test_rect_host.py).  Bars are the project's:
    operator        1e-5 * (scale * max|u| + max|k_sq u| + max|src|), scale = max |L64(normalised noise)| of that shape   (tests/spectral_probes.py)
    transposition   4e-6 * scale * max|u|: two fp32 routes of one operator
    one step        1e-5 * max of each tensor, or 2 x the fp32 oracle's own distance where that exceeds 5e-6               (tests/test_config_matrix.py)
    30 iterations   wavefield <= max(1e-4 * scale, 2 x the fp32 oracle's distance) and <= 4e-4 * scale, scale = max |wf64|; rmse_hist within 2 % of
                    the fp32 oracle's trace
    exact           torch.equal; RMSE rows rtol 1e-5 (one atomicAdd per block: the order of the partial sums is not fixed)
Caller tensors off the 16-byte grid: torch.equal wherever the same kernels run (aligned views between guard words against the plain call; offsets 1, 2,
3 among themselves; every offset against the plain call with the 16-byte-gated kernels switched off); against the plain call with the default options
the route changes: at (32, 80) only conv_state_applies stands down and the bits stay (torch.equal); at (64, 256) dc_asm_applies does too, and there
the bar is the one between two fp32 routes, 4e-6 of max.  RMSE rows rtol 1e-5.
The depth-5 network runs at (32, 96), not at (32, 80): 80 is not a multiple of 2^5, and hn_set_domain_rect asks of each side what hn_set_domain asks
of n (test_contract_arguments asserts that (32, 80) is refused at depth 5).

Spectral lines per block (rect_lines of hn_spectral_line.hip: 16 at most, 80 KB of line buffers at most, halved while ceil(count / lines) * batch
< 512): 1 wherever count * batch < 1024, which is every solver case here and, with its four probes, most of the operator cases; the operator cases
with 2048 or 2032 lines run their short axis at 16 lines per block and (1040, 48) its row pass at 8.  A batch of 3 does not change the lines per
block at (32, 80) or (144, 64), so test_a_sample_does_not_depend_on_its_batch adds the spectral pair at batch 384, where both passes take 16.
"""
import ctypes

import numpy as np
import pytest
import torch

import rect_common as R
import spectral_probes as SP
from caller_buffers import Carved
from config_weights import config_weights
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3
ROUTE_RECT = 5

OPERATOR_SHAPES = [(16, 32), (32, 16), (48, 80), (80, 48), (144, 64), (64, 272), (256, 96), (96, 512), (1040, 48), (16, 2048), (2048, 16), (2032, 16)]
TRANSPOSE_SHAPES = [(48, 80), (144, 64)]
SQUARE_SIZES = [96, 256]
# (16, 512): the kernels of W >= 256 on a very short H (level 3 is 2 x 64 on the streaming conv_state kernel, the bottleneck 1 x 32)
# (256, 512): H >> 3 = 32 and W >> 3 = 64, the sizes at which the deep-level kernels take a square; W >= 256: the hand-scheduled level-0 kernels
STEP_SHAPES = [(32, 80, 2), (80, 32, 2), (16, 48, 1), (64, 256, 1), (256, 64, 1), (48, 272, 1), (16, 512, 1), (256, 512, 1)]
ROUTE_SHAPES = [(32, 80, 2), (256, 512, 1)]
# options that select something a square domain alone has (captured iterations, the side stream and its device words, the deep-level kernels, zero-copy
# histories, the merged level-0 launch, the input layer's sigma map), each away from its default
SQUARE_ONLY_OPTIONS = [("graph", 1, 0), ("side_stream", 0, 1), ("side_stream", 2, 1), ("side_stream", 3, 1), ("deep", 0, 2), ("hist_copy", 1, 0),
                       ("dc_pair", 0, 1), ("side_sync", 0, 1), ("inc_sigma_map", 0, 1)]      # (name, value, default)
LOOP_SHAPES = [(96, 160, 2), (160, 96, 1)]
# batch 384 at (144, 64): columns 144 long, 64 of them -> 64 * 384 / 16 = 1536 blocks >= 512: 16 lines per block; rows 64 long, 144 of them: 16 too
BATCH_SHAPES = [(32, 80, 3), (144, 64, 3), (144, 64, 384)]
GUARD_SHAPES = [(32, 80), (64, 256)]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _engine(h=None, w=None, blob=None, depth=4, act="prelu", precision=None):
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    if blob is not None:
        e.load_weights(blob, 8, depth, 2, act)
    if precision:
        e.set_unet_precision(precision)
    if h is not None:
        e.set_domain_rect(h, w, *R.DOMAIN)
        assert h == w or e.counter("spectral_route") == ROUTE_RECT
    return e


@pytest.fixture(scope="module")
def blob(weights_np):
    from helmnet_amd.engine import pack_weights
    return pack_weights(weights_np, 4, "prelu")


@pytest.fixture(scope="module")
def eng(blob):
    e = _engine(blob=blob)
    yield e
    e.close()


def _err(e):
    return e.lib.hn_last_error(e.ctx).decode()


# ------------------------------------------------------------------------------------------------------------------------------ 1: operator
@pytest.mark.parametrize("h,w", OPERATOR_SHAPES)
def test_operator_matches_the_float64_oracle(eng, h, w):
    c = R.forward_case(h, w)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    assert eng.counter("spectral_route") == ROUTE_RECT
    u, kq = c["u"].to(DEV), c["k_sq"].to(DEV)
    got = {"lap": eng.laplacian(u), "res1": eng.residual(u, kq, c["src1"].to(DEV)), "resb": eng.residual(u, kq, c["srcb"].to(DEV))}
    worst = {}
    for name in got:
        assert not bool(torch.isnan(got[name]).any()), name
        ratio = SP.errors(got[name], c[name]) / c["bar_" + name]
        worst[name] = float(ratio.max())
        print(f"RECT {h}x{w} {name}: error / bar per probe " + ", ".join(f"{p} {float(r):.3f}" for p, r in zip(R.PROBES, ratio)))
    print(f"RECT {h}x{w} (P, Q) rows {R.factor(w)} columns {R.factor(h)}: worst error / bar {max(worst.values()):.3f}")
    assert max(worst.values()) <= 1.0, worst
    # the sigma maps and the flat-state length of the shape
    assert torch.equal(eng.sigmas().cpu(), R.tables(h, w, R.DOMAIN, torch.float32).sigmas)
    assert eng.state_len == R.state_len(h, w)
    # hn_rmse on the rectangular plane
    rm = eng.rmse(got["res1"]).cpu().double()
    want = got["res1"].cpu().double().pow(2).mean((1, 2, 3)).sqrt()
    assert float(((rm - want).abs() / want).max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------- 2: transposition
@pytest.mark.parametrize("h,w", TRANSPOSE_SHAPES)
def test_transposed_domain_gives_the_transposed_laplacian(eng, h, w):
    c = R.forward_case(h, w)
    u = c["u"].to(DEV)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    a = eng.laplacian(u)
    eng.set_domain_rect(w, h, *R.DOMAIN)
    b = eng.laplacian(u.transpose(-1, -2).contiguous()).transpose(-1, -2)
    err = SP.peak(a.cpu().double() - b.cpu().double())
    bar = 4e-6 * c["scale"] * SP.peak(c["u"])
    print(f"RECT {h}x{w} against {w}x{h} transposed: error / bar " + ", ".join(f"{float(r):.3f}" for r in err / bar))
    assert bool((err <= bar).all()), (err / bar).tolist()


# --------------------------------------------------------------------------------------------------------------------------- 3: the square
def _three_steps(e, n, b=2):
    ti = R.teacher_inputs(n, n, b, 300 + n)
    g = {k: v.to(DEV) for k, v in ti.items()}
    k_sq = ((1.0 / g["sos"]) ** 2).contiguous()
    src = R.point_source_map(n, n, [n // 4, n // 2], 10.0).to(DEV)
    res0 = e.residual(g["wf"], k_sq, src)
    wf, res, st = g["wf"].clone(), res0.clone(), g["states"].clone()
    hist = [torch.full((3,) + tuple(t.shape), float("nan"), device=DEV) for t in (res, wf, st)]
    rmse = torch.full((3, b), float("nan"), device=DEV)
    e.step(wf, res, st, k_sq, src, 3, hist[0], hist[1], hist[2], rmse)
    torch.cuda.synchronize()
    e.check_async_errors()
    return [res0, wf, res, st, rmse] + hist


@pytest.mark.parametrize("n", SQUARE_SIZES)
def test_square_is_hn_set_domain_itself(blob, n):
    a, b = _engine(blob=blob), _engine(blob=blob)
    try:
        rc = a.lib.hn_set_domain_rect(a.ctx, n, n, R.PML, R.SIGMA_MAX, R.K)
        assert rc == OK, _err(a)
        a.n, a.hw = n, (n, n)
        b.set_domain(n, *R.DOMAIN)
        assert a.counter("spectral_route") == b.counter("spectral_route") != ROUTE_RECT
        assert a.state_len == b.state_len
        for i, (x, y) in enumerate(zip(_three_steps(a, n), _three_steps(b, n))):
            assert not bool(torch.isnan(x).any())
            if i == 4:      # the RMSE rows: one atomicAdd per block
                assert torch.allclose(x, y, rtol=1e-5, atol=0)
            else:
                assert torch.equal(x, y), i
    finally:
        a.close()
        b.close()


# ----------------------------------------------------------------------------------------------------------------- 4: one teacher-forced step
def _vs_float64(name, got, w64, w32, report):
    """tests/test_config_matrix.py: L_inf <= 1e-5 * max of the float64 result, or 2 x the fp32 oracle's own distance where that is above 5e-6."""
    scale = w64.abs().max().item()
    err = (got.detach().cpu().double() - w64).abs().max().item() / scale
    ora = (w32.double() - w64).abs().max().item() / scale
    bar = 1e-5 if ora <= 5e-6 else 2 * ora
    report.append(f"{name}: {err:.2e} (fp32 oracle {ora:.2e}, bar {bar:.2e})")
    return err <= bar


def _oracle_step(ti, wts, h, w, dtype, depth=4, act="prelu", sd=None):
    t = R.tables(h, w, R.DOMAIN, dtype)
    wd = {k: v.to(dtype) for k, v in wts.items()}
    x = {k: v.to(dtype) for k, v in ti.items()}
    src = R.point_source_map(h, w, [h // 4, w // 2], 10.0).to(dtype)
    k_sq, _ = O.get_initials(x["sos"], 1.0)
    st = R.unflatten_states(x["states"], h, w, depth)
    with torch.no_grad():
        sig = t.sigmas.to(dtype).unsqueeze(0).repeat(x["wf"].shape[0], 1, 1, 1)
        d, _ = O.unet_forward(torch.cat([x["wf"], 1e3 * x["res"], sig], 1), st, wd, depth, act, state_depth=sd)
        wf, res, st2 = O.single_step(x["wf"], k_sq, x["res"], st, wd, src, t, depth, act, state_depth=sd)
    return {"d": d, "wf": wf, "res": res, "states": O.flatten_states(st2)}


def _gpu_step(e, ti, h, w):
    g = {k: v.to(DEV) for k, v in ti.items()}
    k_sq = ((1.0 / g["sos"]) ** 2).contiguous()
    src = R.point_source_map(h, w, [h // 4, w // 2], 10.0).to(DEV)
    sig = e.sigmas().unsqueeze(0).repeat(g["wf"].shape[0], 1, 1, 1)
    d, _ = e.unet(torch.cat([g["wf"], 1e3 * g["res"], sig], 1).contiguous(), g["states"])
    wf, res, st = g["wf"].clone(), g["res"].clone(), g["states"].clone()
    e.step(wf, res, st, k_sq, src, 1)
    torch.cuda.synchronize()
    return {"d": d, "wf": wf, "res": res, "states": st}


def _check_step(tag, e, wts, h, w, b, depth=4, act="prelu", sd=None, seed=0):
    sd_eff = depth if sd is None else sd
    ti = R.teacher_inputs(h, w, b, 9000 + 7 * h + w + seed, depth)
    got = _gpu_step(e, ti, h, w)
    w64, w32 = (_oracle_step(ti, wts, h, w, dt, depth, act, sd) for dt in (torch.float64, torch.float32))
    report, ok = [], []
    for k in ("d", "wf", "res"):
        ok.append(_vs_float64(k, got[k], w64[k], w32[k], report))
    o = 0
    for d in range(depth):
        lv = slice(o, o + (h >> d) * (w >> d))
        o = lv.stop
        if d < sd_eff:
            ok.append(_vs_float64(f"state{d}", got["states"][:, :, lv], w64["states"][:, :, lv], w32["states"][:, :, lv], report))
    print(f"RECT step [{tag}] " + "; ".join(report))
    assert all(ok), report


@pytest.mark.parametrize("h,w,b", STEP_SHAPES)
def test_one_teacher_forced_step_vs_float64(eng, weights, h, w, b):
    eng.set_domain_rect(h, w, *R.DOMAIN)
    _check_step(f"{h}x{w}x{b}", eng, weights, h, w, b)


def test_one_step_in_the_valu_mode(blob, weights):
    e = _engine(32, 80, blob, precision="valu")
    try:
        _check_step("32x80x2 valu", e, weights, 32, 80, 2)
    finally:
        e.close()


@pytest.mark.parametrize("tag,depth,act,sd,h,w", [("d2relu", 2, "relu", None, 32, 80), ("d5", 5, "prelu", None, 32, 96), ("d4sd2", 4, "prelu", 2, 32, 80)])
def test_one_step_on_other_networks(tag, depth, act, sd, h, w):
    from helmnet_amd.engine import pack_weights
    wn = config_weights(depth, 770 + depth, "A" if act == "prelu" else None, act, sd, n=min(h, w))
    wts = {k: torch.from_numpy(v) for k, v in wn.items()}
    e = _engine(h, w, pack_weights(wn, depth, act, sd), depth, act)
    try:
        assert e.state_len == R.state_len(h, w, depth)
        _check_step(f"{h}x{w}x2 {tag}", e, wts, h, w, 2, depth, act, sd)
    finally:
        e.close()


# -------------------------------------------------------------------------------------------------------------------------------- 5: the loop
@pytest.mark.parametrize("h,w,b", LOOP_SHAPES)
def test_thirty_iterations_from_rest(eng, weights, h, w, b):
    n_iter = 30
    wf64, tr64 = R.oracle_loop(h, w, b, n_iter, weights, torch.float64)
    wf32, tr32 = R.oracle_loop(h, w, b, n_iter, weights, torch.float32)
    eng.set_domain_rect(h, w, *R.DOMAIN)
    k_sq = ((1.0 / R.box_sos(h, w, b)) ** 2).to(DEV).contiguous()
    src = R.point_source_map(h, w, [h // 4, w // 2], 10.0).to(DEV)
    wf = torch.zeros(b, 2, h, w, device=DEV)
    res = eng.residual(wf, k_sq, src)
    st = torch.zeros(b, 2, eng.state_len, device=DEV)
    rmse = torch.full((n_iter, b), float("nan"), device=DEV)
    eng.step(wf, res, st, k_sq, src, n_iter, rmse_hist=rmse)
    torch.cuda.synchronize()
    scale = wf64.abs().max().item()
    err, ora = (wf.cpu().double() - wf64).abs().max().item(), (wf32.double() - wf64).abs().max().item()
    rel = ((rmse.cpu().double() - tr32.double()).abs() / tr32.double()).max().item()
    print(f"RECT loop {h}x{w}x{b} 30 it: Linf vs float64 {err:.3e}, fp32 oracle {ora:.3e}, |wf| {scale:.3e}; rmse_hist vs fp32 oracle {rel:.2e}; "
          f"last rmse {rmse[-1].tolist()}")
    assert err <= max(1e-4 * scale, 2 * ora) and err <= 4e-4 * scale
    assert rel <= 0.02


# ---------------------------------------------------------------------------------------------------------------------- 6: exact properties
def _problem(h, w, b, seed):
    ti = R.teacher_inputs(h, w, b, seed)
    g = {k: v.to(DEV) for k, v in ti.items()}
    return {"wf": g["wf"], "res": g["res"], "states": g["states"], "k_sq": ((1.0 / g["sos"]) ** 2).contiguous(),
            "src": R.point_source_map(h, w, [h // 4, w // 2], 10.0).to(DEV), "ti": ti}


def _run(e, p, n_iter, idx=None, hist=False):
    sel = (lambda t: t.clone()) if idx is None else (lambda t: t[idx].clone().contiguous())
    wf, res, st, kq = sel(p["wf"]), sel(p["res"]), sel(p["states"]), sel(p["k_sq"])
    b = wf.shape[0]
    rmse = torch.full((n_iter, b), float("nan"), device=DEV)
    hs = [torch.full((n_iter,) + tuple(t.shape), float("nan"), device=DEV) for t in (res, wf, st)] if hist else [None, None, None]
    e.step(wf, res, st, kq, p["src"], n_iter, hs[0], hs[1], hs[2], rmse)
    torch.cuda.synchronize()
    return dict(wf=wf, res=res, st=st, rmse=rmse, res_hist=hs[0], wf_hist=hs[1], st_hist=hs[2])


@pytest.mark.parametrize("h,w,b", BATCH_SHAPES)
def test_a_sample_does_not_depend_on_its_batch(eng, h, w, b):
    eng.set_domain_rect(h, w, *R.DOMAIN)
    p3 = _problem(h, w, 3, 41 + h)
    if b == 3:
        many, one = _run(eng, p3, 2), _run(eng, p3, 2, idx=[1])
        for k in ("wf", "res", "st"):
            assert torch.equal(many[k][1], one[k][0]), k
        assert torch.allclose(many["rmse"][:, 1], one["rmse"][:, 0], rtol=1e-5, atol=0)
    else:      # the spectral pair alone at a batch that moves both passes to 16 lines per block (a UNet workspace for 384 samples is not needed for that)
        u, kq = p3["wf"], p3["k_sq"]
        idx = [j % 3 for j in range(b)]
        one = [eng.residual(u[i:i + 1], kq[i:i + 1], p3["src"])[0] for i in range(3)]
        many = eng.residual(u[idx].contiguous(), kq[idx].contiguous(), p3["src"])
        for j in (0, 1, 2, b - 2, b - 1):
            assert torch.equal(many[j], one[idx[j]]), j


def test_iterations_in_one_call_or_in_several(eng):
    h, w = 32, 80
    eng.set_domain_rect(h, w, *R.DOMAIN)
    p = _problem(h, w, 2, 77)
    four = _run(eng, p, 4, hist=True)
    again = _run(eng, p, 4, hist=True)
    for k in four:                                   # two calls on equal inputs
        assert not bool(torch.isnan(four[k]).any()), k
        if k == "rmse":
            assert torch.allclose(four[k], again[k], rtol=1e-5, atol=0)
        else:
            assert torch.equal(four[k], again[k]), k
    cur = dict(p)
    rows = []
    for t in range(4):                               # four calls of one: slot t of every history is the state after t + 1 single calls
        o = _run(eng, cur, 1)
        cur = dict(cur, wf=o["wf"], res=o["res"], states=o["st"])
        rows.append(o["rmse"][0])
        assert torch.equal(four["wf_hist"][t], o["wf"]) and torch.equal(four["res_hist"][t], o["res"]) and torch.equal(four["st_hist"][t], o["st"]), t
    assert torch.equal(four["wf"], cur["wf"]) and torch.equal(four["res"], cur["res"]) and torch.equal(four["st"], cur["states"])
    assert torch.allclose(four["rmse"], torch.stack(rows), rtol=1e-5, atol=0)
    a = _run(eng, p, 2)                              # 2 + 2
    bb = _run(eng, dict(p, wf=a["wf"], res=a["res"], states=a["st"]), 2)
    assert torch.equal(bb["wf"], four["wf"]) and torch.equal(bb["res"], four["res"]) and torch.equal(bb["st"], four["st"])
    assert torch.allclose(torch.cat([a["rmse"], bb["rmse"]]), four["rmse"], rtol=1e-5, atol=0)
    want = four["res_hist"].double().pow(2).mean((2, 3, 4)).sqrt()      # the fused RMSE rows are those of their residual slots
    assert float(((four["rmse"].double() - want).abs() / want).max()) <= 1e-5


def _carved_step(e, p, n_iter, k):
    """hn_step with every tensor a view k floats past a 16-byte boundary between guard words (k = 0: aligned, still between guard words)."""
    b, (h, w) = p["wf"].shape[0], p["wf"].shape[-2:]
    new = lambda *s: torch.zeros(s)  # noqa: E731
    tensors = {"wf": p["wf"].cpu(), "res": p["res"].cpu(), "states": p["states"].cpu(), "k_sq": p["k_sq"].cpu(), "src": p["src"].cpu(),
               "res_hist": new(n_iter, b, 2, h, w), "wf_hist": new(n_iter, b, 2, h, w), "st_hist": new(n_iter, b, 2, e.state_len), "rmse": new(n_iter, b)}
    c = Carved(tensors, DEV, offsets={name: k for name in tensors})
    e.step(c["wf"], c["res"], c["states"], c["k_sq"], c["src"], n_iter, c["res_hist"], c["wf_hist"], c["st_hist"], c["rmse"])
    torch.cuda.synchronize()
    c.check()
    for name in GUARD_FIELDS:
        assert not bool(torch.isnan(c[name]).any()), (k, name)
    return c


GUARD_FIELDS = {"wf": "wf", "res": "res", "states": "st", "res_hist": "res_hist", "wf_hist": "wf_hist", "st_hist": "st_hist"}    # Carved name -> _run name


@pytest.mark.parametrize("h,w", GUARD_SHAPES)
def test_caller_tensors_off_the_16_byte_grid_between_guard_words(eng, blob, weights, h, w):
    """The convention of tests/test_caller_buffers_gpu.py: exact bits wherever the same kernels run, the bar between two fp32 routes (4e-6 of max) only
    where the arithmetic really changes, the RMSE rows rtol 1e-5 throughout, and the off-grid run against the float64 oracle.  With the default options
    a pointer off the 16-byte grid changes the route: conv_state_applies (levels at least 64 wide, both shapes; same bits on either kernel) and
    dc_asm_applies (W >= 256: (64, 256); other bits) ask for 16 bytes and stand down."""
    eng.set_domain_rect(h, w, *R.DOMAIN)
    b, n_iter = 2, 2
    p = _problem(h, w, b, 55 + w)
    plain = _run(eng, p, n_iter, hist=True)
    # aligned views between guard words: the kernels of the plain call
    c0 = _carved_step(eng, p, n_iter, 0)
    for name, pn in GUARD_FIELDS.items():
        assert torch.equal(c0[name], plain[pn]), name
    assert torch.allclose(c0["rmse"], plain["rmse"], rtol=1e-5, atol=0)
    # offsets 1, 2 and 3: the same kernels among themselves, the same bits
    off = {k: _carved_step(eng, p, n_iter, k) for k in (1, 2, 3)}
    for k in (2, 3):
        for name in GUARD_FIELDS:
            assert torch.equal(off[k][name], off[1][name]), (k, name)
        assert torch.allclose(off[k]["rmse"], off[1]["rmse"], rtol=1e-5, atol=0)
    # off the grid against the plain call: another route, the bar between two fp32 routes
    print(f"RECT off-grid {h}x{w}: fields with other bits than the plain call: " + ", ".join(n for n, pn in GUARD_FIELDS.items() if not torch.equal(off[1][n], plain[pn])))
    for name, pn in GUARD_FIELDS.items():
        if w < 256:     # only conv_state changes its kernel, and the streaming kernel sums in the direct kernel's order: the issue's torch.equal
            assert torch.equal(off[1][name], plain[pn]), name
        else:           # the hand-scheduled DoubleConvs stand down: other arithmetic
            assert (off[1][name] - plain[pn]).abs().max().item() <= 4e-6 * plain[pn].abs().max().item(), name
    assert torch.allclose(off[1]["rmse"], plain["rmse"], rtol=1e-5, atol=0)
    # the kernels that ask for 16 bytes switched off (no streaming conv_state, no hand-scheduled / packed-FMA DoubleConvs): the route cannot change,
    # and every offset gives the bits of the plain call
    e = _engine(h, w, blob)
    try:
        e.set_option("state_kernel", 0)
        e.set_option("dc_valu", 0)
        base = _run(e, p, n_iter, hist=True)
        for k in (1, 3):
            ck = _carved_step(e, p, n_iter, k)
            for name, pn in GUARD_FIELDS.items():
                assert torch.equal(ck[name], base[pn]), (k, name)
            assert torch.allclose(ck["rmse"], base["rmse"], rtol=1e-5, atol=0)
    finally:
        e.close()
    # one step off the grid against the float64 oracle
    one = _carved_step(eng, p, 1, 1)
    w64, w32 = (_oracle_step(p["ti"], weights, h, w, dt) for dt in (torch.float64, torch.float32))
    report, ok = [], []
    for name, key in (("wf", "wf"), ("res", "res"), ("states", "states")):
        ok.append(_vs_float64(name, one[name], w64[key], w32[key], report))
    print(f"RECT off-grid step {h}x{w}: " + "; ".join(report))
    assert all(ok), report
    # the operator entry points on such views
    lap = Carved({"u": p["wf"].cpu(), "out": torch.zeros(b, 2, h, w)}, DEV, offsets={"u": 1, "out": 3})
    assert eng.lib.hn_laplacian(eng.ctx, _ptr(lap["u"]), _ptr(lap["out"]), b, eng._stream()) == OK, _err(eng)
    torch.cuda.synchronize()
    lap.check()
    assert torch.equal(lap["out"], eng.laplacian(p["wf"]))


def test_live_buffer_as_slot_0_of_its_history(eng):
    """hn_step's one tolerated overlap, res_hist == res and wf_hist == wf: slot 0 and the live buffer are one piece of memory and end up holding the
    last iteration's value; the other slots hold their iterations."""
    h, w, b, n_iter = 32, 80, 2, 3
    eng.set_domain_rect(h, w, *R.DOMAIN)
    p = _problem(h, w, b, 63)
    plain = _run(eng, p, n_iter, hist=True)
    wf_hist = torch.full((n_iter, b, 2, h, w), float("nan"), device=DEV)
    res_hist = torch.full_like(wf_hist, float("nan"))
    wf_hist[0].copy_(p["wf"])
    res_hist[0].copy_(p["res"])
    st = p["states"].clone()
    eng.step(wf_hist[0], res_hist[0], st, p["k_sq"], p["src"], n_iter, res_hist, wf_hist, None, None)
    torch.cuda.synchronize()
    assert torch.equal(wf_hist[0], plain["wf"]) and torch.equal(res_hist[0], plain["res"]) and torch.equal(st, plain["st"])
    for t in range(1, n_iter):
        assert torch.equal(wf_hist[t], plain["wf_hist"][t]) and torch.equal(res_hist[t], plain["res_hist"][t]), t


def test_second_call_can_be_captured_and_replayed(blob):
    h, w = 32, 80
    e = _engine(h, w, blob)
    try:
        p = _problem(h, w, 2, 91)
        eager = _run(e, p, 2)                        # (builds the workspace)
        wf, res, st = p["wf"].clone(), p["res"].clone(), p["states"].clone()
        rmse = torch.full((2, 2), float("nan"), device=DEV)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = e.lib.hn_step(e.ctx, _ptr(wf), _ptr(res), _ptr(st), _ptr(p["k_sq"]), _ptr(p["src"]), 1, 2, 2, None, None, None, _ptr(rmse), e._stream())
            assert rc == OK, _err(e)
            wf.copy_(p["wf"]); res.copy_(p["res"]); st.copy_(p["states"])
            graph.replay()
            torch.cuda.synchronize()
        assert torch.equal(wf, eager["wf"]) and torch.equal(res, eager["res"]) and torch.equal(st, eager["st"])
        assert torch.allclose(rmse, eager["rmse"], rtol=1e-5, atol=0)
    finally:
        e.close()


@pytest.mark.parametrize("h,w,b", ROUTE_SHAPES)
def test_square_only_options_do_not_move_a_rectangle_off_its_route(blob, h, w, b):
    """A rectangle runs one lane, launched kernel by kernel on the caller's stream, with copied histories, whatever the options of the square path say:
    the same bits, no captured iteration, no flag-synchronised one, no stream probe, and every iteration counted as launched one by one.
    The RMSE rows keep this file's rtol 1e-5 (one atomicAdd per block: two runs of one route need not give the same bits there); they are also the
    RMSE of the residual history, which is compared exactly."""
    n_iter = 8
    still = ("graph_replays", "graphs_captured", "flag_sync_iterations", "stream_probes")
    e = _engine(h, w, blob)
    try:
        p = _problem(h, w, b, 29 + w)

        def counted_run():
            before = {k: e.counter(k) for k in still + ("eager_iterations",)}
            out = _run(e, p, n_iter, hist=True)
            e.check_async_errors()
            moved = {k: e.counter(k) - v for k, v in before.items()}
            assert moved.pop("eager_iterations") == n_iter
            assert not any(moved.values()), moved
            return out

        base = counted_run()
        for k in base:
            assert not bool(torch.isnan(base[k]).any()), k
        for name, value, default in SQUARE_ONLY_OPTIONS:
            e.set_option(name, value)
            got = counted_run()
            e.set_option(name, default)
            for k in base:
                if k == "rmse":
                    assert torch.allclose(got[k], base[k], rtol=1e-5, atol=0), (name, value)
                else:
                    assert torch.equal(got[k], base[k]), (name, value, k)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7: contract
def test_contract_arguments(blob):
    from helmnet_amd.engine import pack_weights
    e = _engine(blob=blob)
    try:
        sd = lambda h, w, pml=R.PML: e.lib.hn_set_domain_rect(e.ctx, h, w, pml, R.SIGMA_MAX, R.K)  # noqa: E731
        for h, w in ((40, 64), (64, 40), (0, 64), (64, 8), (2064, 64), (64, 4096)):
            assert sd(h, w) == ERR_ARG, (h, w)
        assert sd(64, 16, 9) == ERR_ARG and sd(16, 64, 9) == ERR_ARG and sd(64, 32, 0) == ERR_ARG      # 2 * pml must fit each axis; pml >= 1
        assert sd(64, 16, 8) == OK and e.counter("spectral_route") == ROUTE_RECT
    finally:
        e.close()
    wn = config_weights(5, 775, "A", "prelu", None, n=32)
    e = _engine(blob=pack_weights(wn, 5, "prelu"), depth=5)
    try:
        assert e.lib.hn_set_domain_rect(e.ctx, 32, 80, R.PML, R.SIGMA_MAX, R.K) == ERR_ARG       # 80 is not a multiple of 2^5
        assert e.lib.hn_set_domain_rect(e.ctx, 32, 96, R.PML, R.SIGMA_MAX, R.K) == OK
    finally:
        e.close()


def test_refused_entry_points_write_nothing(blob):
    h, w, b = 32, 80, 1
    e = _engine(h, w, blob)
    try:
        p = _problem(h, w, b, 13)
        L = e.state_len
        nan32 = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        nan64 = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float64)  # noqa: E731
        f64 = {k: p[k].double() for k in ("wf", "res", "states", "k_sq", "src")}
        n_w = int(e.lib.hn_weight_count(8, 4, 2))
        wts = torch.from_numpy(np.ascontiguousarray(blob)).to(DEV)
        hist = [p["wf"][None].clone(), p["res"][None].clone(), p["states"][None].clone()]
        outs = []

        def refused(name, call, *written):
            with pytest.raises(NotImplementedError, match="rectangular domain"):
                call()
            outs.extend(written)

        o, o64 = nan32(b, 2, h, w), nan64(b, 2, h, w)
        assert e.lib.hn_residual_vjp(e.ctx, _ptr(p["wf"]), _ptr(p["k_sq"]), _ptr(o), b, e._stream()) == ERR_UNSUPPORTED and "rectangular domain" in _err(e)
        assert e.lib.hn_laplacian_f64(e.ctx, _ptr(f64["wf"]), _ptr(o64), b, e._stream()) == ERR_UNSUPPORTED and "rectangular domain" in _err(e)
        outs.extend([o, o64])
        # the entry points whose outputs the Engine wrappers allocate: through the C ABI into NaN-filled outputs (in-place ones: unchanged inputs)
        lib, st, z = e.lib, e._stream(), None
        r64, m64, so64, d64 = nan64(b, 2, h, w), nan64(b), nan64(b, 2, L), nan64(b, 2, h, w)
        in6 = torch.zeros(b, 6, h, w, device=DEV, dtype=torch.float64)
        assert lib.hn_residual_f64(e.ctx, _ptr(f64["wf"]), _ptr(f64["k_sq"]), _ptr(f64["src"]), 1, _ptr(r64), _ptr(m64), b, st) == ERR_UNSUPPORTED
        assert lib.hn_unet_f64(e.ctx, _ptr(in6), _ptr(f64["states"]), _ptr(so64), _ptr(d64), b, st) == ERR_UNSUPPORTED and "rectangular domain" in _err(e)
        s64 = [f64[k].clone() for k in ("wf", "res", "states")]
        assert lib.hn_step_f64(e.ctx, _ptr(s64[0]), _ptr(s64[1]), _ptr(s64[2]), _ptr(f64["k_sq"]), _ptr(f64["src"]), 1, b, 1, z, z, z, _ptr(m64), st) == ERR_UNSUPPORTED
        tg = [nan32(2, b, 2, h, w), nan32(2, b, 2, h, w), nan32(2, b, 2, L), nan32(1), nan32(n_w), nan32(b, 2, h, w), nan32(b, 2, h, w), nan32(b, 2, L)]
        assert lib.hn_train_grad(e.ctx, _ptr(wts), _ptr(p["wf"]), _ptr(p["res"]), _ptr(p["states"]), _ptr(p["k_sq"]), _ptr(p["src"]), 1, b, 2, 1e4,
                                 *[_ptr(t) for t in tg], st) == ERR_UNSUPPORTED and "rectangular domain" in _err(e)
        gv = [nan32(b, 2, h, w), nan32(b, 2, h, w), nan32(b, 2, L), nan32(b, 1, h, w), nan32(1, 2, h, w), nan32(n_w)]
        assert lib.hn_step_vjp(e.ctx, _ptr(wts), _ptr(p["wf"]), _ptr(p["res"]), _ptr(p["states"]), _ptr(p["k_sq"]), 1, b, 1, *[_ptr(t) for t in hist],
                               z, z, z, _ptr(p["wf"]), z, z, *[_ptr(t) for t in gv], 0, st) == ERR_UNSUPPORTED and "rectangular domain" in _err(e)
        torch.cuda.synchronize()
        assert all(torch.equal(a, f64[k]) for a, k in zip(s64, ("wf", "res", "states")))
        outs.extend([r64, m64, so64, d64] + tg + gv)
        refused("hn_residual_vjp", lambda: e.residual_vjp(p["wf"], p["k_sq"]))
        refused("hn_laplacian_f64", lambda: e.laplacian64(f64["wf"]))
        refused("hn_residual_f64", lambda: e.residual64(f64["wf"], f64["k_sq"], f64["src"]))
        refused("hn_unet_f64", lambda: e.unet64(torch.zeros(b, 6, h, w, device=DEV, dtype=torch.float64), f64["states"]))
        refused("hn_step_f64", lambda: e.step64(f64["wf"].clone(), f64["res"].clone(), f64["states"].clone(), f64["k_sq"], f64["src"], 1))
        x = p["wf"].clone()
        refused("hn_gmres_cycle", lambda: e.gmres_cycle(x, p["k_sq"], p["src"], 4, 1e-6))
        refused("hn_fgmres_cycle", lambda: e.fgmres_cycle(x, p["k_sq"], p["src"], 4, 1e-6, 2, 1.0))
        x64 = f64["wf"].clone()
        refused("hn_gmres_refine_cycle", lambda: e.gmres_refine_cycle(x64, p["k_sq"], p["src"], 4, 1e-9))
        refused("hn_fgmres_refine_cycle", lambda: e.fgmres_refine_cycle(x64, p["k_sq"], p["src"], 4, 1e-9, 2, 1.0))
        refused("hn_train_reserve", lambda: e.train_reserve(b, 2))
        refused("hn_train_grad", lambda: e.train_grad(wts, p["wf"], p["res"], p["states"], p["k_sq"], p["src"], 2))
        refused("hn_step_vjp", lambda: e.step_vjp(wts, p["wf"], p["res"], p["states"], p["k_sq"], 1, *hist, g_wf_T=p["wf"]))
        t_wf, t_res, t_st = nan32(b, 2, h, w), nan32(b, 2, h, w), nan32(b, 2, L)
        refused("hn_step_jvp", lambda: e.step_jvp(p["wf"], p["res"], p["states"], p["k_sq"], 1, *hist, t_wf, t_res, t_st), t_wf, t_res, t_st)
        wf2, res2, st2, kq2, src2 = (p[k].clone() for k in ("wf", "res", "states", "k_sq", "src"))
        refused("hn_stream_swap", lambda: e.stream_swap(wf2, res2, st2, kq2, src2, [[0, -1, -1, 0]], torch.ones(1, 1, h, w, device=DEV)))
        assert torch.equal(x, p["wf"]) and torch.equal(x64, f64["wf"]) and torch.equal(wf2, p["wf"]) and torch.equal(kq2, p["k_sq"])
        assert n_w == wts.numel()
        # the 16-bit modes: hn_unet and hn_step
        for mode in ("fp16", "bf16x3", "bf16x2"):
            e.set_unet_precision(mode)
            wf, res, st = p["wf"].clone(), p["res"].clone(), p["states"].clone()
            with pytest.raises(NotImplementedError, match="rectangular domain"):
                e.step(wf, res, st, p["k_sq"], p["src"], 1)
            with pytest.raises(NotImplementedError, match="rectangular domain"):
                e.unet(torch.zeros(b, 6, h, w, device=DEV), p["states"])
            torch.cuda.synchronize()
            assert torch.equal(wf, p["wf"]) and torch.equal(res, p["res"]) and torch.equal(st, p["states"])
        e.set_unet_precision("fp32")
        e.set_option("lanes", 2)
        with pytest.raises(NotImplementedError, match="rectangular domain"):
            e.step(p["wf"].clone(), p["res"].clone(), p["states"].clone(), p["k_sq"], p["src"], 1)
        e.set_option("lanes", 1)
        torch.cuda.synchronize()
        for t in outs:
            assert bool(torch.isnan(t).all())
        # hn_step's overlap refusal
        wf = p["wf"].clone()
        with pytest.raises(ValueError, match="overlaps"):
            e.step(wf, wf, p["states"].clone(), p["k_sq"], p["src"], 1)
    finally:
        e.close()


def test_first_step_under_capture_is_refused_and_reserve_lifts_it(blob):
    h, w = 32, 80
    e = _engine(h, w, blob)
    try:
        p = _problem(h, w, 1, 17)
        wf, res, st = p["wf"].clone(), p["res"].clone(), p["states"].clone()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                rc = e.lib.hn_step(e.ctx, _ptr(wf), _ptr(res), _ptr(st), _ptr(p["k_sq"]), _ptr(p["src"]), 1, 1, 1, None, None, None, None, e._stream())
        torch.cuda.synchronize()
        assert rc == ERR_STATE, (rc, _err(e))
        assert "capture" in _err(e)
        assert torch.equal(wf, p["wf"]) and torch.equal(st, p["states"])
        e.reserve(1)
        e.step(wf, res, st, p["k_sq"], p["src"], 1)
        torch.cuda.synchronize()
        assert not torch.equal(wf, p["wf"])
    finally:
        e.close()


def test_square_domain_after_a_rectangular_one(blob):
    n = 96
    a, fresh = _engine(32, 80, blob), _engine(blob=blob)
    try:
        _run(a, _problem(32, 80, 1, 5), 1)
        a.set_domain(n, *R.DOMAIN)
        fresh.set_domain(n, *R.DOMAIN)
        assert a.counter("spectral_route") == fresh.counter("spectral_route") != ROUTE_RECT
        ti = R.teacher_inputs(n, n, 2, 23)
        g = {k: v.to(DEV) for k, v in ti.items()}
        p = {"wf": g["wf"], "res": g["res"], "states": g["states"], "k_sq": ((1.0 / g["sos"]) ** 2).contiguous(),
             "src": R.point_source_map(n, n, [n // 4, n // 2], 10.0).to(DEV)}
        x, y = _run(a, p, 1), _run(fresh, p, 1)
        for k in ("wf", "res", "st"):
            assert torch.equal(x[k], y[k]), k
    finally:
        a.close()
        fresh.close()


def test_python_front_end():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    h, w = 96, 160
    s.set_domain_size((h, w), source_location=[h // 4, w // 2])
    sos = R.box_sos(h, w, 2).to(DEV)
    out = s.forward(sos, num_iterations=3, return_wavefields=True, return_states=True)
    assert set(out) >= {"wavefields", "residuals", "states", "last_iteration"} and out["last_iteration"] == 2
    assert all(tuple(t.shape) == (2, 2, h, w) for t in out["wavefields"] + out["residuals"]) and len(out["wavefields"]) == len(out["residuals"]) == 3
    assert tuple(out["states"][0].shape) == (2, 2, R.state_len(h, w))
    assert [tuple(t.shape[-2:]) for t in s.f.get_states()] == [(h >> d, w >> d) for d in range(4)]
    assert tuple(s.sigmas.shape) == (2, h, w) and torch.equal(s.sigmas.cpu(), s.engine().sigmas().cpu())
    k_sq, wf = s.get_initials(sos)
    assert tuple(s.apply_laplacian(out["wavefields"][-1]).shape) == (2, 2, h, w)
    assert torch.equal(s.get_residual(out["wavefields"][-1], k_sq), out["residuals"][-1])
    tol = s.solve_to_tolerance(sos, tol=1e-4, max_iterations=400, check_every=25)
    print(f"RECT python: solve_to_tolerance(1e-4) at {h}x{w}: {tol['iterations']} iterations, converged {tol['converged']}, "
          f"last rmse {tol['residual_norms'][-1].tolist()}")
    assert tol["converged"] and tol["iterations"] < 400
    for name, call in (("forward64", lambda: s.forward64(sos)), ("verify", lambda: s.verify(wf, sos_maps=sos)), ("gmres", lambda: s.gmres(sos)),
                       ("gmres64", lambda: s.gmres64(sos)), ("solve_many", lambda: s.solve_many(sos, 1e-3)), ("trainer", lambda: s.trainer()),
                       ("jvp", lambda: s.jvp(sos, d_sos=torch.ones_like(sos))), ("fp16", lambda: s.set_unet_precision("fp16")),
                       ("deviation", lambda: s.deviation_from_float64(sos, 4, [2])), ("reference_error", lambda: s.reference_error(wf, sos)),
                       ("autograd", lambda: s.forward(sos.clone().requires_grad_(True), num_iterations=2))):
        with pytest.raises(NotImplementedError, match="rectangular domain"):
            call()
    s.set_domain_size(96, source_location=[20, 48])      # and back to a square
    assert s.engine().counter("spectral_route") == 2
