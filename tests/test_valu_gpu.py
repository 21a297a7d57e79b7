"""The direct fp32 kernels (k_double_conv, k_down8x8, k_up8x8 of hn_unet.hip) on a real MI355X: the whole network in HN_PREC_FP32_VALU on square
domains against the float64 oracle, and the three sub-module entry points (hn_double_conv, hn_conv8x8, hn_out_conv) against a float64
F.conv2d composition at every (cin, cout), every activation and the shapes around one tile.

These kernels are the header's "A/B reference for the matrix-core kernels", the whole UNet of a rectangular domain and the fall-back of
conv_state; before this file they ran on a GPU at one rectangle (32 x 80) and, standalone, on PReLU at four shapes.

Bars.  Whole network: the _vs_float64 form of tests/test_config_matrix.py (1e-5 * max of the float64 result, or 2 x the fp32 oracle's own distance
where that is above 5e-6), and within 4e-6 * max of the fp32 matrix-core mode without being equal to it.  Sub-modules: 1e-5 * max for the
piecewise-linear activations (the bar of test_sub_modules_called_directly_match_the_oracle); the smooth ones take the _vs_float64 form, the
fp32 CPU composition of the same layers standing in for the oracle.

Measured on an MI355X (of max |float64|; in brackets the fp32 CPU oracle / composition against float64):
  whole network, worst of d, wf, res and the levels' states: ship_16 1.67e-06 (1.24e-06), ship_48 1.53e-06 (1.35e-06), ship_80 1.22e-06 (9.89e-07),
    ship_272 1.41e-06 (9.87e-07), d2_64 9.85e-07 (8.89e-07), d5_96 1.58e-06 (1.57e-06), d4_80_sd2 1.26e-06 (1.36e-06), gelu 7.21e-07 (1.22e-06),
    softplus 6.14e-07 (6.15e-07); from the matrix-core mode 2.2e-06 at most (res at 272^2), never equal
  hn_double_conv, worst over the five channel pairs and eight shapes: prelu 4.74e-07 (4.50e-07), relu 3.60e-07 (3.79e-07), leakyrelu 4.46e-07
    (4.68e-07), celu 4.25e-07 (3.90e-07), tanh 4.78e-07 (4.18e-07), gelu 5.30e-07 (4.95e-07), tanhshrink 4.32e-07 (4.88e-07), softplus 4.21e-07
    (4.35e-07): the composition's own distance never exceeds 5e-6, so the smooth activations are held to 1e-5 as well
  hn_conv8x8 stride 2 1.09e-06, transposed 5.12e-07; hn_out_conv 1.02e-07
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from config_solver import DEV, _solver, _step, _unet
from config_weights import GPU_CONFIGS, config_input, config_weights
from oracle import helmnet_oracle as O
from test_config_matrix import _levels, _oracle, _vs_float64

pytestmark = pytest.mark.gpu

# tag -> (depth, weight seed (None: the shipped checkpoint), slope plan, activation, state_depth, n, batch)
VALU_NETS = {
    "ship_16": (4, None, None, "prelu", 4, 16, 3),        # a 1 x 1 deepest plane, 2 x 2 -> 1 x 1 stride-2 convolutions
    "ship_48": (4, None, None, "prelu", 4, 48, 3),        # a 3 x 3 bottleneck, odd planes
    "ship_80": (4, None, None, "prelu", 4, 80, 2),        # levels 80 / 40 / 20 / 10 / 5
    "ship_272": (4, None, None, "prelu", 4, 272, 1),      # partial 16 x 32 tiles both ways at levels 1 (136) and 2 (68)
    "d2_64": GPU_CONFIGS["d2_64"],
    "d5_96": (5, 760, "A", "prelu", 5, 96, 2),
    "d4_80_sd2": (4, 748, "B", "prelu", 2, 80, 2),        # levels 2 and 3 without state: their slots keep their bits
    "d4_48_gelu": (4, 741, None, "gelu", 4, 48, 2),       # the smooth epilogue of the direct kernel
    "d4_48_softplus": (4, 741, None, "softplus", 4, 48, 2),
}


@pytest.mark.parametrize("tag", list(VALU_NETS))
def test_whole_network_in_valu_mode_vs_float64(tag, weights_np):
    depth, seed, plan, act, sd, n, b = VALU_NETS[tag]
    w = weights_np if seed is None else config_weights(depth, seed, plan, act, sd, n=n)
    c = dict(depth=depth, act=act, sd=sd, n=n, b=b, w=w, x=config_input(n, b, depth, 9400 + n, wf_scale=1e-6))
    got = {}
    for mode in ("valu", "fp32"):
        s = _solver(depth, act, sd, w, n, mode=mode)
        eng = s.engine()
        assert eng.unet_precision == mode
        if mode == "valu":
            eng.profile_enable(None)
            _step(s, c["x"])
            torch.cuda.synchronize()
            names = set(eng.profile_collect())
            eng.profile_enable([])
            assert not ({"deep", "inc_conv_signal0"} & names), sorted(names)
            assert {"inc", "bottleneck"} | {f"conv_signal{d}" for d in range(depth)} | {f"up{d}" for d in range(depth)} <= names, sorted(names)
        out = dict(zip(("wf", "res", "states"), _step(s, c["x"])))
        out["d"] = _unet(s, c["x"])
        torch.cuda.synchronize()
        eng.check_async_errors()
        got[mode] = {k: v.cpu() for k, v in out.items()}
    idx = list(range(b))
    w64, w32 = _oracle(c, torch.float64, idx), _oracle(c, torch.float32, idx)
    report, ok = [], []
    for k in ("d", "wf", "res"):
        ok.append(_vs_float64(k, got["valu"][k], w64[k], w32[k], report))
    x_st = torch.from_numpy(c["x"]["states"])
    for d, lv in enumerate(_levels(n, depth)):
        if d < sd:
            ok.append(_vs_float64(f"state{d}", got["valu"]["states"][:, :, lv], w64["states"][:, :, lv], w32["states"][:, :, lv], report))
        else:
            assert torch.equal(got["valu"]["states"][:, :, lv], x_st[:, :, lv]), d
    # two fp32 implementations: not the same bits (the direct kernels ran, not the matrix-core ones), the header's 4e-6 * max apart at most
    gap = {k: ((got["valu"][k] - got["fp32"][k]).abs().max() / got["fp32"][k].abs().max()).item() for k in ("d", "wf", "res", "states")}
    print(f"[valu {tag}] " + "; ".join(report) + "; vs the matrix-core mode " + ", ".join(f"{k} {v:.1e}" for k, v in gap.items()))
    assert all(ok), report
    assert not all(torch.equal(got["valu"][k], got["fp32"][k]) for k in gap), tag
    assert max(gap.values()) <= 4e-6, gap


# ------------------------------------------------------------------------------------------------------------------ the sub-module entry points
ACTS = ("prelu", "relu", "leakyrelu", "celu", "tanh", "gelu", "tanhshrink", "softplus")
PAIRS = ((6, 8), (8, 8), (10, 8), (16, 8), (10, 2))
SLOPES = (-0.4, 0.3, 1.6, -1.2, 2.5)         # PReLU: both sides of 0 and of 1, one per (cin, cout)
# DcCfg: 16 rows x 16 / 32 / 64 columns (by width).  1 x 1 and 2 x 2; exactly one tile and one past it both ways, for each tile width
DC_SHAPES = ((1, 1), (2, 2), (16, 16), (17, 17), (16, 32), (17, 33), (16, 64), (17, 65))
DOWN_SHAPES = ((2, 2), (16, 32), (32, 64), (34, 66), (38, 50))       # DownCfg: 16 x 32 OUTPUTS per tile; 38 x 50 gives odd output planes 19 x 25
UP_SHAPES = ((1, 1), (16, 32), (17, 33), (37, 50))                   # UpCfg: 16 x 32 INPUTS per tile
BATCH = 3
PAYLOAD = 0x7FC0BEEF


@pytest.fixture(scope="module")
def eng():
    from helmnet_amd.engine import Engine
    e = Engine(torch.device(DEV))
    yield e
    e.close()


def _rel(got, w64):
    return ((got.detach().cpu().double() - w64).abs().max() / w64.abs().max()).item()


def _dc_weights(g, cin, cout):
    w1 = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    w2 = torch.randn(cout, cout, 3, 3, generator=g) / (9 * cout) ** 0.5 * 1.4
    return w1, 0.3 * torch.randn(cout, generator=g), w2, 0.3 * torch.randn(cout, generator=g)


def _dc_ref(x, w1, b1, slope, w2, b2, act, dtype):
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    h = F.conv2d(x, w1, b1, padding=1)
    if act in ("prelu", "relu", "leakyrelu"):     # the slope is the fp32 value the blob carries
        h = torch.where(h > 0, h, torch.tensor(np.float32(slope).item(), dtype=dtype) * h)
    else:
        h = O.activation(h, act, None)
    return F.conv2d(h, w2, b2, padding=1)


@pytest.mark.parametrize("act", ACTS)
def test_double_conv_every_channel_pair_and_shape_vs_float64(eng, act):
    g = torch.Generator().manual_seed(4100 + ACTS.index(act))
    smooth = act not in ("prelu", "relu", "leakyrelu")
    worst, worst_ora = 0.0, 0.0
    for (cin, cout), prelu_slope in zip(PAIRS, SLOPES):
        slope = {"prelu": prelu_slope, "relu": 0.0, "leakyrelu": 0.01}.get(act, 0.0)
        w1, b1, w2, b2 = _dc_weights(g, cin, cout)
        for h, w in DC_SHAPES:
            x = 1.5 * torch.randn(BATCH, cin, h, w, generator=g)
            got = eng.double_conv(x.to(DEV), w1, b1, slope, w2, b2, activation=act)
            w64 = _dc_ref(x, w1, b1, slope, w2, b2, act, torch.float64)
            err = _rel(got, w64)
            ora = _rel(_dc_ref(x, w1, b1, slope, w2, b2, act, torch.float32), w64)
            bar = 2 * ora if (smooth and ora > 5e-6) else 1e-5
            worst, worst_ora = max(worst, err), max(worst_ora, ora)
            assert got.shape == (BATCH, cout, h, w) and err <= bar, (act, cin, cout, h, w, err, ora, bar)
    print(f"[double_conv {act}] worst {worst:.2e} of max |float64| (fp32 CPU composition {worst_ora:.2e})")


def test_conv8x8_and_out_conv_vs_float64(eng):
    g = torch.Generator().manual_seed(4200)
    wd, bd = torch.randn(8, 8, 8, 8, generator=g) / 512 ** 0.5, 0.3 * torch.randn(8, generator=g)
    wu, bu = torch.randn(8, 8, 8, 8, generator=g) / 128 ** 0.5, 0.3 * torch.randn(8, generator=g)
    wo, bo = torch.randn(2, 8, 1, 1, generator=g) / 8 ** 0.5, 0.3 * torch.randn(2, generator=g)
    worst = {"down": 0.0, "up": 0.0, "out": 0.0}
    for h, w in DOWN_SHAPES:
        x = torch.randn(BATCH, 8, h, w, generator=g)
        got = eng.conv8x8(x.to(DEV), wd, bd, transposed=False)
        w64 = F.conv2d(x.double(), wd.double(), bd.double(), stride=2, padding=3)
        assert got.shape == w64.shape == (BATCH, 8, h // 2, w // 2)
        worst["down"] = max(worst["down"], _rel(got, w64))
        assert _rel(got, w64) <= 1e-5, ("down", h, w, _rel(got, w64))
    for h, w in UP_SHAPES:
        x = torch.randn(BATCH, 8, h, w, generator=g)
        got = eng.conv8x8(x.to(DEV), wu, bu, transposed=True)
        w64 = F.conv_transpose2d(x.double(), wu.double(), bu.double(), stride=2, padding=3)
        assert got.shape == w64.shape == (BATCH, 8, 2 * h, 2 * w)
        worst["up"] = max(worst["up"], _rel(got, w64))
        assert _rel(got, w64) <= 1e-5, ("up", h, w, _rel(got, w64))
    for h, w in ((1, 1), (2, 2), (16, 32), (17, 33), (37, 50)):
        x = torch.randn(BATCH, 8, h, w, generator=g)
        got = eng.out_conv(x.to(DEV), wo, bo)
        w64 = F.conv2d(x.double(), wo.double(), bo.double())
        worst["out"] = max(worst["out"], _rel(got, w64))
        assert got.shape == w64.shape and _rel(got, w64) <= 1e-5, ("out", h, w, _rel(got, w64))
    print("[conv8x8 / out_conv] worst of max |float64|: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_refusals_leave_out_untouched(eng):
    """Another (cin, cout), an odd plane for the stride-2 form and an activation kind outside hn_act: HN_ERR_UNSUPPORTED, nothing enqueued, every
    word of ``out`` still the NaN payload it was filled with."""
    UNSUPPORTED = -3
    x = torch.randn(1, 16, 17, 16, device=DEV)
    out = torch.empty(8 * 34 * 32, device=DEV)
    out.view(torch.int32).fill_(PAYLOAD)
    blob = np.zeros(8192, np.float32)          # (more than any of the three weight layouts reads)
    fp = blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    lib, stream = eng.lib, eng._stream()
    calls = {
        "(4, 8)": lambda: lib.hn_double_conv(eng.ctx, ptr(x), 4, 8, fp, 0, ptr(out), 1, 16, 16, stream),
        "(8, 2)": lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 2, fp, 0, ptr(out), 1, 16, 16, stream),
        "act_kind 8": lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 8, fp, 8, ptr(out), 1, 16, 16, stream),
        "act_kind -1": lambda: lib.hn_double_conv(eng.ctx, ptr(x), 8, 8, fp, -1, ptr(out), 1, 16, 16, stream),
        "odd h": lambda: lib.hn_conv8x8(eng.ctx, ptr(x), fp, 0, ptr(out), 1, 17, 16, stream),
        "odd w": lambda: lib.hn_conv8x8(eng.ctx, ptr(x), fp, 0, ptr(out), 1, 16, 17, stream),
    }
    for what, call in calls.items():
        assert call() == UNSUPPORTED, what
        assert lib.hn_last_error(eng.ctx), what
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == PAYLOAD).all()), what
    # the transposed form takes the odd plane the stride-2 form refused
    assert lib.hn_conv8x8(eng.ctx, ptr(x), fp, 1, ptr(out), 1, 17, 16, stream) == 0
    torch.cuda.synchronize()
    assert bool((out[: 8 * 34 * 32] == 0).all())          # zero weights, zero bias
