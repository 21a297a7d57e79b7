"""The network's DoubleConv / 8x8 dispatch one layer at a time on a real MI355X: hn_double_conv / hn_conv8x8 with 'module_mc' 1 run launch_dc8 /
launch_down / launch_up on the call's weights, so every matrix-core instance of hn_mfma.hip (and hn_dcv.hip, hn_dca.hip) is held to a float64
F.conv2d / F.conv_transpose2d composition by itself, at one tile, one tile and a bit, and several tiles and a part with H != W (tests/mc_layers.py: TABLE).

  routes   hn_module_route names the instance the table expects, at every plane and setting: each leg below asserts it beside its result
  exact    small-integer operands (and impulses against all-different weights): torch.equal to the float64 reference in fp32 with 'mc_stage' 0 and 1,
           bf16x3, fp16 and bf16x2 (tests/test_mc_layers_host.py holds the preconditions); a failure names the first wrong element and its tile
  random   (two bars do not carry over to a single small layer: see below)  the generators and bars of tests/test_valu_gpu.py: 1e-5 * max |float64| for prelu / relu / leakyrelu, the _vs_float64 form (2 x the fp32 CPU
           composition's own distance where that is above 5e-6, else 1e-5) for gelu / softplus; within 4e-6 * max of the direct kernels ('module_mc' 0,
           the header's bar between two fp32 kernel sets) without being equal to them in every tensor; 'mc_stage' 0 and 1 bit-equal on the ring
           instances' planes.  16-bit modes: the rule of tests/test_x16_gpu.py (x16_oracle.accept, and the rms ratio that shows the 16-bit kernel
           ran) against x16_oracle.q_double_conv / q_conv8 on inputs fp16 represents exactly, as there
  guards   x and out as views between guard words, 4 bytes past / 12 bytes past a 16-byte boundary (hn_dca.hip: aligned, and a misaligned call gives the
           bits of hn_dcv.hip): the result is still the reference, every guard word intact; a NaN sample 1 leaves sample 0's bits alone

Two places where a bar of the files above does not carry over to one small layer, and what stands there instead:
  * k_dc_mfma_p and k_dc_mfma add up every output in the direct kernel's order (the f32 matrix instruction is a chain of fused multiply-adds), so on
    finite data they ARE equal to the 'module_mc' 0 result in every tensor (0.0e+00 in all 456 cases below).  "Not equal, so the direct kernel did not
    run" cannot hold for them; where a row is equal everywhere, the test demands the other proof that the matrix core ran: one +Inf in the input
    reaches, as 0 * Inf = NaN through the zero that fills the fourth slot of a 3-tap row in the fragment packing, a pixel the direct kernel keeps finite.
  * fp16 DoubleConv: "max error <= 2 x the twin's" and "rms ratio >= half the twin's" compare two handfuls of flipped fp16 units of the mid tensor; on
    planes of 2 k to 7 k pixels those are one or two flips each (twin max 4.6e-06 .. 1.7e-04, twin ratio 23 .. 930 over the 16 cases; GPU 3.1e-05
    against a twin of 1.3e-05 at 16 x 128 x 8 channels).  As the issue rules for a bar that does not apply: the rounded oracle's own distance from
    the unrounded float64 composition is measured on the same case and twice that is allowed, beside the unchanged "at most 2 % beyond 1e-5", and
    the ratio has to show the result closer to the rounded oracle than to the unrounded one (> 1).  bf16x3, bf16x2 and the 8x8 kernels keep the rule as it is.
  The fp16 kernels clamp a NaN input to +-65504 (HalfF16::split: fmin / fmax), so a NaN sample stays finite there; the NaN leg asserts sample 0 only.

Measured on an MI355X, worst over the planes and channel counts of each instance, of max |float64| (in brackets the fp32 CPU composition on the same
cases; then the distance from the direct kernels, bar 4e-6):
  dc_asm 5.59e-07 (5.02e-07) 5.3e-07; dc_valu 4.83e-07 (4.57e-07) 4.8e-07; k_dc_mfma_s 5.62e-07 (4.75e-07) 4.8e-07; k_dc_mfma_s_gen 5.36e-07 (4.96e-07)
  4.8e-07; k_dc_mfma_s_ring 4.55e-07 (4.68e-07) 4.2e-07; k_dc_mfma_p_32 4.86e-07 (4.43e-07) 0; k_dc_mfma_p_16 4.83e-07 (4.45e-07) 0; k_dc_mfma_64
  4.72e-07 (5.33e-07) 0; k_dc_mfma_32 5.70e-07 (4.59e-07) 0; k_dc_mfma_16 4.15e-07 (5.00e-07) 0; down_64 4.46e-07 (9.18e-07) 9.1e-07; down_ring_64
  6.10e-07 (9.16e-07) 1.0e-06; down_32 4.61e-07 (1.09e-06) 9.4e-07; down_ring_32 5.01e-07 (8.45e-07) 1.2e-06; down_16 5.19e-07 (8.40e-07) 7.3e-07;
  up_2_11 4.17e-07 (5.07e-07) 3.0e-07; up_ring 4.29e-07 (3.94e-07) 3.2e-07; up_1_5 4.42e-07 (4.52e-07) 3.2e-07
  16-bit, of max |rounded oracle| (twin): k_dc_x16_bf16x3 3.48e-07 (4.84e-07); k_dc_x16_bf16x2 4.80e-06 (4.11e-06); k_dc_x16_fp16 1.47e-04 (1.66e-04),
  beyond 1e-5 at most 0.34 %; down_x16 fp16 1.98e-07 (8.28e-07), bf16x2 2.69e-07 (9.80e-07); up_x16 bf16x3 3.79e-07 (6.75e-07), fp16 1.99e-07
  (4.90e-07), bf16x2 2.44e-07 (5.60e-07)
Every exact and impulse leg is equal bit for bit in all five settings (and on hn_dcv.hip / hn_dca.hip); the file runs in 6 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import mc_layers as M
import x16_oracle as X
from caller_buffers import margins_intact, offset_view
from config_solver import DEV
from helmnet_amd import _lib
from test_valu_gpu import SLOPES as VALU_SLOPES
from test_valu_gpu import _dc_ref, _dc_weights, _rel

pytestmark = pytest.mark.gpu

EXACT_ROWS = [k for k, r in M.TABLE.items() if r.op != "double_conv_smooth"]
FP32_SETTINGS = ("fp32_s0", "fp32_s1", "fp32_valu", "fp32_asm")


@pytest.fixture(scope="module")
def engines():
    """{needs weights: Engine}: a bare context, and a solver's (weights loaded: hn_dca.hip's zero page)."""
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    bare = Engine(torch.device(DEV))
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    s.set_domain_size(64, source_location=[16, 32])
    loaded = s.engine()
    yield {False: bare, True: loaded}
    M.restore(loaded)
    bare.close()


def _engine(engines, setting, module_mc=1):
    eng = engines[M.SETTINGS[setting][3]]
    M.apply_setting(eng, setting, module_mc)
    return eng


def _settings(inst):
    return M.FIVE + M.EXTRA.get(inst, ())


def _check_route(eng, inst, row, setting, cin, plane):
    """Where the table says the instance is reached, hn_module_route must name it; -> whether it is."""
    if cin not in row.reached.get(setting, ()):
        return False
    assert eng.module_route(row.op, cin, *plane) == inst, (inst, setting, cin, plane, eng.module_route(row.op, cin, *plane))
    return True


# ------------------------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("inst", list(M.TABLE))
def test_route_of_every_table_case(engines, inst):
    row = M.TABLE[inst]
    n = 0
    for setting, cins in row.reached.items():
        eng = _engine(engines, setting)
        for plane in row.planes:
            for cin in cins:
                n += _check_route(eng, inst, row, setting, cin, plane)
        eng.set_option("module_mc", 0)
        assert eng.module_route(row.op, cins[0], *row.planes[0]) == "direct"
        eng.set_option("module_mc", 1)
        eng.set_unet_precision("valu")
        assert eng.module_route(row.op, cins[0], *row.planes[0]) == "direct"
    assert n >= 3
    for eng in engines.values():
        M.restore(eng)


def test_route_refusals(engines):
    eng = _engine(engines, "fp32_s1")
    for op, cin, h, w in ((4, 8, 16, 16), (-1, 8, 16, 16), (0, 7, 16, 16), (1, 10, 16, 16), (2, 6, 16, 16), (0, 8, 0, 16), (1, 8, 17, 16), (1, 8, 16, 17)):
        assert eng.lib.hn_module_route(eng.ctx, op, cin, h, w) == -1, (op, cin, h, w)
    assert eng.lib.hn_module_route(eng.ctx, 2, 8, 17, 17) == _lib.HN_ROUTE["up_1_5"]
    M.restore(eng)


# ------------------------------------------------------------------------------------------------------------------ exact legs
def _run_exact(engines, inst, cases_of):
    """cases_of(cin, plane) -> list of cases; every case in every setting of the row must equal its float64 reference bit for bit."""
    row = M.TABLE[inst]
    reached, cases = 0, cases_of(row)
    for setting in _settings(inst):
        eng = _engine(engines, setting)
        for plane, cin, case in cases:
            reached += _check_route(eng, inst, row, setting, cin, plane)
            got = M.run(eng, row, case, DEV)
            torch.cuda.synchronize()
            bad = M.first_mismatch(row, got, case["want"])
            assert not bad, f"{inst} {setting} cin {cin} plane {plane} (route {eng.module_route(row.op, cin, *plane)}): {bad}"
    assert reached >= 1, inst
    for eng in engines.values():
        M.restore(eng)


@pytest.mark.parametrize("inst", EXACT_ROWS)
def test_small_integer_operands_give_the_float64_reference_bit_for_bit(engines, inst):
    _run_exact(engines, inst, lambda row: [(p, c, M.exact_case(inst, c, p)) for p in row.planes for c in row.cins])


@pytest.mark.parametrize("inst", EXACT_ROWS)
def test_an_impulse_returns_the_weight_slice_bit_for_bit(engines, inst):
    _run_exact(engines, inst, lambda row: [(row.big, c, case) for c in row.cins for case in M.impulse_cases(inst, c, row.big)])


# ------------------------------------------------------------------------------------------------------------------ random-valued legs, fp32
def _fp32_settings(inst, row):
    s = [t for t in FP32_SETTINGS if t in row.reached]
    if inst in M.RING and "fp32_s0" not in s:
        s.insert(0, "fp32_s0")        # the kernel the ring instance replaced: its bits are the contract
    return s


def _random_case(row, g, cin, plane, act, slope):
    b = row.batch(plane)
    if row.op in ("double_conv", "double_conv_smooth"):
        w1, b1, w2, b2 = _dc_weights(g, cin, 8)
        x = 1.5 * torch.randn(b, cin, *plane, generator=g)
        w64 = _dc_ref(x, w1, b1, slope, w2, b2, act, torch.float64)
        ora = _rel(_dc_ref(x, w1, b1, slope, w2, b2, act, torch.float32), w64)
        return dict(x=x, args=(w1, b1, slope, w2, b2), act=act), w64, ora
    up = row.op == "up"
    wt, bias = torch.randn(8, 8, 8, 8, generator=g) / (128 if up else 512) ** 0.5, 0.3 * torch.randn(8, generator=g)
    x = torch.randn(b, 8, *plane, generator=g)
    w64 = M.k8_ref(x, wt, bias, up)
    return dict(x=x, args=(wt, bias)), w64, _rel(M.k8_ref(x, wt, bias, up, torch.float32), w64)


def _inf_footprint_differs(engines, row, setting, cin, plane):
    """Which kernel ran, where the bits cannot tell.  k_dc_mfma_p and k_dc_mfma add up every output in the direct kernel's order (input channel, row,
    tap, one fused multiply-add each: the f32 matrix instruction is that chain), so on finite data they return its bits.  But the matrix core takes a
    3-tap row as FOUR products, the fourth against a zero of the fragment packing (pack_frag_3x3): with one +Inf in the input, 0 * Inf = NaN reaches a
    pixel whose 3 x 3 window does not hold it, a product the direct kernel never forms.  -> whether the sets of non-finite outputs differ."""
    g = torch.Generator().manual_seed(5150)
    w1, b1, w2, b2 = _dc_weights(g, cin, 8)
    x = torch.zeros(2, cin, *plane)
    x[0, 0, plane[0] // 2, plane[1] // 2] = float("inf")
    case = dict(x=x, args=(w1, b1, 0.3, w2, b2), act="prelu")
    masks = [~torch.isfinite(M.run(_engine(engines, setting, module_mc=mc), row, case, DEV)) for mc in (0, 1)]
    assert bool(masks[0][0].any()) and not bool(masks[0][1].any()) and not bool(masks[1][1].any())      # (and sample 1 stays finite under both)
    return not torch.equal(masks[0], masks[1])


@pytest.mark.parametrize("inst", [k for k, r in M.TABLE.items() if any(s in r.reached for s in FP32_SETTINGS)])
def test_random_values_in_fp32_vs_float64_and_the_direct_kernels(engines, inst):
    row = M.TABLE[inst]
    g = torch.Generator().manual_seed(5100 + sorted(M.TABLE).index(inst))
    acts = {"double_conv": ("prelu", "relu", "leakyrelu"), "double_conv_smooth": ("gelu", "softplus")}.get(row.op, (None,))
    settings = _fp32_settings(inst, row)
    worst, worst_ora, worst_gap, equal_everywhere, n = 0.0, 0.0, 0.0, True, 0
    for act in acts:
        for cin in row.cins:
            slope = {"prelu": VALU_SLOPES[M.ALL_CIN.index(cin)] if cin in M.ALL_CIN else 0.3, "relu": 0.0, "leakyrelu": 0.01}.get(act, 0.0)
            for plane in row.planes:
                case, w64, ora = _random_case(row, g, cin, plane, act, slope)
                smooth = row.op == "double_conv_smooth"
                bar = 2 * ora if (smooth and ora > 5e-6) else 1e-5
                direct = M.run(_engine(engines, settings[0], module_mc=0), row, case, DEV)
                got = {}
                for setting in settings:
                    eng = _engine(engines, setting)
                    on_inst = _check_route(eng, inst, row, setting, cin, plane)
                    if not on_inst and not (inst in M.RING and setting == "fp32_s0"):
                        continue
                    got[setting] = M.run(eng, row, case, DEV)
                    torch.cuda.synchronize()
                    err = _rel(got[setting], w64)
                    gap = ((got[setting] - direct).abs().max() / direct.abs().max()).item()
                    assert got[setting].shape == w64.shape and err <= bar, (inst, setting, act, cin, plane, err, ora, bar)
                    assert gap <= 4e-6, (inst, setting, act, cin, plane, gap)
                    if on_inst:
                        worst, worst_ora, worst_gap, n = max(worst, err), max(worst_ora, ora), max(worst_gap, gap), n + 1
                        equal_everywhere = equal_everywhere and torch.equal(got[setting], direct)
                if inst in M.RING and "fp32_s1" in got:      # the existing contract of 'mc_stage', at layer level and on H != W
                    assert torch.equal(got["fp32_s0"], got["fp32_s1"]), (inst, act, cin, plane)
    print(f"[{inst}] {n} cases, worst {worst:.2e} of max |float64| (fp32 CPU composition {worst_ora:.2e}), from the direct kernels {worst_gap:.1e}")
    assert n >= 3, inst
    if equal_everywhere:       # the same bits in every tensor: either the direct kernel ran, or the instance sums in the direct kernel's order
        setting = next(s for s in settings if s in row.reached)
        differs = _inf_footprint_differs(engines, row, setting, row.reached[setting][-1], row.big)
        print(f"[{inst}] bit-equal to the direct kernels in all {n} cases; the footprint of one Inf differs from theirs: {differs}")
        assert differs, inst
    for eng in engines.values():
        M.restore(eng)


# ------------------------------------------------------------------------------------------------------------------ random-valued legs, 16 bit
def _exact16(g, shape):
    return torch.randint(-1024, 1025, shape, generator=g).float() / 512.0       # multiples of 2^-9 in [-2, 2], as x16_oracle.exact_input


@pytest.mark.parametrize("inst", [k for k, r in M.TABLE.items() if "x16" in k])
def test_random_values_in_the_16_bit_modes_vs_the_rounded_oracle(engines, inst):
    row = M.TABLE[inst]
    g = torch.Generator().manual_seed(5200 + sorted(M.TABLE).index(inst))
    bad, lines, worst = [], [], {}
    for mode, cins in row.reached.items():
        for cin in cins:
            for plane in row.planes:
                b = row.batch(plane)
                x = _exact16(g, (b, cin, *plane))
                if row.op == "double_conv":
                    w1, b1, w2, b2 = _dc_weights(g, cin, 8)
                    slope = VALU_SLOPES[M.ALL_CIN.index(cin)]
                    w = {"l.double_conv.0.weight": w1, "l.double_conv.0.bias": b1, "l.double_conv.1.weight": torch.tensor([slope]),
                         "l.double_conv.2.weight": w2, "l.double_conv.2.bias": b2}
                    case = dict(x=x, args=(w1, b1, slope, w2, b2), act="prelu")
                    want, twin = X.q_double_conv(x, w, "l", "prelu", mode), X.q_double_conv(x, w, "l", "prelu", mode, acc=torch.float32)
                    plain = _dc_ref(x, w1, b1, slope, w2, b2, "prelu", torch.float64)
                else:
                    up = row.op == "up"
                    wt, bias = torch.randn(8, 8, 8, 8, generator=g) / (128 if up else 512) ** 0.5, 0.3 * torch.randn(8, generator=g)
                    case = dict(x=x, args=(wt, bias))
                    want, twin = X.q_conv8(x, wt, bias, mode, up), X.q_conv8(x, wt, bias, mode, up, acc=torch.float32)
                    plain = M.k8_ref(x, wt, bias, up)
                eng = _engine(engines, mode)
                assert _check_route(eng, inst, row, mode, cin, plane)
                got = M.run(eng, row, case, DEV).cpu()
                ok, fig = X.accept(mode, got, want, twin)
                line = f"{mode} cin {cin} {plane}: gpu max {fig['max']:.2e} (twin {fig['twin_max']:.2e})"
                if mode == "fp16":
                    line += f", beyond 1e-5 {fig['over']:.2%} (twin {fig['twin_over']:.2%})"
                    if row.op == "double_conv":      # (module docstring: the 2 x twin part of the rule does not carry over to a single small DoubleConv)
                        fmt = float(X.errors(want, plain).max())
                        line += f", oracle from float64 {fmt:.2e}"
                        ok = fig["over"] <= X.FP16_FRACTION and fig["max"] <= 2 * fmt
                worst[mode] = max(worst.get(mode, 0.0), fig["max"])
                if mode != "bf16x3":
                    r_gpu, r_twin = X.rms_ratio(got, want, plain), X.rms_ratio(twin, want, plain)
                    line += f", rms ratio {r_gpu:.1f} (twin {r_twin:.1f})"
                    # (fp16 DoubleConv: a handful of flipped mid units make up the whole denominator, the twin's ratio itself scatters 23 .. 930; closer to
                    #  the rounded oracle than to the unrounded one is what the ratio has to show)
                    ok = ok and (r_gpu > 1.0 if (mode == "fp16" and row.op == "double_conv") else r_gpu >= 0.5 * r_twin)
                else:      # (no rms ratio tells bf16x3 from fp32: the bits do)
                    ref = M.run(_engine(engines, "fp32_s1"), row, case, DEV).cpu()
                    ok = ok and not torch.equal(got, ref)
                lines.append(line)
                if not ok:
                    bad.append(line)
    print(f"[{inst}] worst of max |oracle| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + "\n    " + "\n    ".join(lines))
    M.restore(engines[False])
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ guard words, NaN, refusals
def _raw(eng, row, case, x, out):
    """The C entry point on the caller's own x and out (Engine.double_conv / conv8x8 allocate out themselves)."""
    b, cin, h, w = x.shape
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))      # noqa: E731
    with torch.cuda.device(eng.device):
        if row.op in ("double_conv", "double_conv_smooth"):
            w1, b1, slope, w2, b2 = case["args"]
            blob = eng._host_blob([w1, b1, np.float32([slope]), w2, b2])
            rc = eng.lib.hn_double_conv(eng.ctx, ptr(x), cin, 8, fp(blob), _lib.HN_ACT[case["act"]], ptr(out), b, h, w, eng._stream())
        else:
            blob = eng._host_blob(list(case["args"]))
            rc = eng.lib.hn_conv8x8(eng.ctx, ptr(x), fp(blob), int(row.op == "up"), ptr(out), b, h, w, eng._stream())
    _lib.check(rc, eng.ctx, row.op)
    torch.cuda.synchronize()


def _nan_payload(shape):
    return torch.full(shape, M.PAYLOAD, dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("inst", EXACT_ROWS)
def test_views_between_guard_words_and_a_nan_sample(engines, inst):
    """On the instance's largest plane (partial tiles both ways): an out-of-image READ would bring the guard word -- a NaN -- into the result, which is
    compared bit for bit; an out-of-image WRITE would change a guard word.  Then sample 1 all NaN: sample 0 keeps its bits."""
    row = M.TABLE[inst]
    setting = next(iter(row.reached))
    cin, plane = row.reached[setting][-1], row.big
    eng = _engine(engines, setting)
    assert _check_route(eng, inst, row, setting, cin, plane)
    case = M.exact_case(inst, cin, plane)
    kx, ko = (0, 0) if inst == "dc_asm" else (1, 3)
    xbuf, x = offset_view(case["x"].to(DEV), kx)
    obuf, out = offset_view(_nan_payload(tuple(case["want"].shape)).to(DEV), ko)
    assert x.data_ptr() % 16 == 4 * kx and out.data_ptr() % 16 == 4 * ko
    _raw(eng, row, case, x, out)
    bad = M.first_mismatch(row, out, case["want"])
    assert not bad, f"{inst} {setting} cin {cin} plane {plane}: {bad}"
    assert margins_intact(xbuf, x) and margins_intact(obuf, out), inst
    first = out.clone()
    x[1] = float("nan")
    _raw(eng, row, case, x, out)
    assert torch.equal(out[0], first[0]) and margins_intact(obuf, out), inst
    M.restore(eng)


def test_a_misaligned_call_leaves_hn_dca_for_hn_dcv(engines):
    """hn_dca.hip stages with 16-byte loads: an x that is only 4-byte aligned takes hn_dcv.hip, bit for bit what 'dc_valu' 2 gives; the aligned call
    differs from it somewhere (two summation orders)."""
    row = M.TABLE["dc_asm"]
    g = torch.Generator().manual_seed(5300)
    cin, plane = 16, (17, 260)
    w1, b1, w2, b2 = _dc_weights(g, cin, 8)
    xc = 1.5 * torch.randn(2, cin, *plane, generator=g)
    case = dict(x=xc, args=(w1, b1, 0.3, w2, b2), act="prelu")
    res = {}
    for name, setting, k in (("asm", "fp32_asm", 0), ("asm_misaligned", "fp32_asm", 1), ("valu", "fp32_valu", 0)):
        eng = _engine(engines, setting)      # (both on the context with weights: the same engine would do, the table's settings say which)
        xbuf, x = offset_view(xc.to(DEV), k)
        obuf, out = offset_view(_nan_payload((2, 8, *plane)).to(DEV), 0)
        _raw(eng, row, case, x, out)
        assert margins_intact(xbuf, x) and margins_intact(obuf, out), name
        res[name] = out.clone()
    assert torch.equal(res["asm_misaligned"], res["valu"])
    assert not torch.equal(res["asm"], res["valu"])
    assert _rel(res["asm"], _dc_ref(xc, w1, b1, 0.3, w2, b2, "prelu", torch.float64)) <= 1e-5
    for eng in engines.values():
        M.restore(eng)


def test_refusals_are_those_of_the_direct_path_and_leave_out_untouched(engines):
    """tests/test_valu_gpu.py's refusals with 'module_mc' 1: the same status, a message, nothing enqueued, every word of out still the NaN payload."""
    eng = _engine(engines, "fp32_s1")
    x = torch.randn(1, 16, 17, 16, device=DEV)
    out = torch.empty(8 * 34 * 32, device=DEV)
    out.view(torch.int32).fill_(M.PAYLOAD)
    blob = np.zeros(8192, np.float32)
    fp = blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    lib, stream = eng.lib, eng._stream()
    calls = {
        "(4, 8)": (-3, lambda: lib.hn_double_conv(eng.ctx, ptr(x), 4, 8, fp, 0, ptr(out), 1, 16, 16, stream)),
        "(8, 2)": (-3, lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 2, fp, 0, ptr(out), 1, 16, 16, stream)),
        "act_kind 8": (-3, lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 8, fp, 8, ptr(out), 1, 16, 16, stream)),
        "act_kind -1": (-3, lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 8, fp, -1, ptr(out), 1, 16, 16, stream)),
        "odd h": (-3, lambda: lib.hn_conv8x8(eng.ctx, ptr(x), fp, 0, ptr(out), 1, 17, 16, stream)),
        "odd w": (-3, lambda: lib.hn_conv8x8(eng.ctx, ptr(x), fp, 0, ptr(out), 1, 16, 17, stream)),
        "batch 0": (-1, lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 8, fp, 0, ptr(out), 0, 16, 16, stream)),
        "NULL x": (-1, lambda: lib.hn_conv8x8(eng.ctx, None, fp, 1, ptr(out), 1, 16, 16, stream)),
    }
    messages = {}
    for mc in (1, 0):
        eng.set_option("module_mc", mc)
        for what, (status, call) in calls.items():
            assert call() == status, (what, mc)
            messages.setdefault(what, []).append(lib.hn_last_error(eng.ctx))
            torch.cuda.synchronize()
            assert bool((out.view(torch.int32) == M.PAYLOAD).all()), (what, mc)
    assert all(m[0] and m[0] == m[1] for m in messages.values()), messages
    # (10, 2) stays on the direct kernel under either value: the same bits
    g = torch.Generator().manual_seed(5400)
    w1, b1, w2, b2 = _dc_weights(g, 10, 2)
    xs = torch.randn(2, 10, 19, 66, generator=g).to(DEV)
    res = []
    for mc in (0, 1):
        eng.set_option("module_mc", mc)
        res.append(eng.double_conv(xs, w1, b1, 0.3, w2, b2))
    assert torch.equal(res[0], res[1])
    M.restore(eng)
