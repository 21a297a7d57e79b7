"""Operand-rounded float64 oracle of the 16-bit UNet modes (fp16 / bf16x2 / bf16x3): what k_dc_x16, k_down_x16 and k_up_x16 of hn_mfma.hip compute,
restated with stock PyTorch CPU ops.  TEST CODE ONLY (a helper beside spectral_probes.py); the spectral parts and every layer that stays in fp32 are those
of oracle/helmnet_oracle.py.

The arithmetic of the kernels:
  * an fp32 operand x is split into parts: bf16 modes p0 = bf16_rne(x), p1 = bf16_rne(x - p0), and for bf16x3 p2 = bf16_rne(x - p0 - p1); fp16 mode the one
    part f16_rne(clamp(x, +-65504)) for activations (HalfF16::split saturates) and f16_rne(w) for weights (packed on the host, not clamped);
  * a product is the sum of the TERMS of the mode, named activation part x weight part (h, m, l = part 0, 1, 2), accumulated in fp32 with fp32 biases;
  * a DoubleConv splits its inputs (the step path multiplies the residual by 1e3 in fp32 first), runs conv1, applies the piecewise-linear activation in
    fp32, splits the mid tensor again (zero outside the image) and runs conv2;
  * which layers do this is `quantised()` below, the rule of launch_dc_mfma / launch_down / launch_up; every other layer is fp32.

``acc`` chooses the accumulator: torch.float64 is the oracle; torch.float32 is the CPU TWIN -- the same rounded operands summed in fp32 in another order than
the kernel's, i.e. to the float64 oracle what a correct kernel is.  Its deviation from the oracle is the scale of the acceptance bars (`accept`).
``Mut`` switches one deliberate bug on; tests/test_x16_host.py shows that every one of them fails the bars.

`passthrough_weights` builds networks in which every layer but one hands its input on exactly (on inputs fp16 represents exactly), so that one layer's
output is seen without another 16-bit layer's rounding flips on top: see the CASES table.
"""
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from config_weights import GPU_CONFIGS, config_input, config_weights
from helmnet_amd.engine import weight_shapes
from oracle import helmnet_oracle as O

MODES = ("fp16", "bf16x2", "bf16x3")
NPARTS = {"fp16": 1, "bf16x2": 2, "bf16x3": 3}
TERMS = {"fp16": ("hh",), "bf16x2": ("hh", "hm", "mh"), "bf16x3": ("hh", "hm", "mh", "mm", "hl", "lh")}
_PART = {"h": 0, "m": 1, "l": 2}
PWL = ("prelu", "relu", "leakyrelu")       # the activations the 16-bit DoubleConv has an epilogue for
F16_MAX = 65504.0


@dataclass(frozen=True)
class Mut:
    """One deliberate bug of the quantised layers (all off: the specification)."""
    drop_term: Optional[str] = None     # leave this product term out
    truncate: bool = False              # activations converted by truncation instead of round-to-nearest-even
    raw_mid: bool = False               # the mid tensor of a DoubleConv enters conv2 unrounded
    drop_halo: bool = False             # conv2 outputs at x = 63 (mod 64) miss the mid column to their right (the next tile's first: "pair column 32")
    no_clamp: bool = False              # fp16 activations are converted without the clamp to +-65504 (an overflow becomes infinity)
    termwise: bool = False              # no bug either: another summation order (one convolution per term, small terms first, channels reversed)
    smooth16: bool = False              # a wrong dispatch, not wrong arithmetic: DoubleConvs with a smooth activation run in 16 bits too


SPEC = Mut()
MUTATIONS = {"truncate": Mut(truncate=True), "raw_mid": Mut(raw_mid=True), "drop_halo": Mut(drop_halo=True)}


def term_mutations(mode):
    """Every single-term mutation of a mode that has more than one term."""
    return {f"drop_{t}": Mut(drop_term=t) for t in TERMS[mode][1:]}


# ------------------------------------------------------------------------------------------
# operand parts
# ------------------------------------------------------------------------------------------
def _to16(r: torch.Tensor, mode: str, truncate: bool) -> torch.Tensor:
    """fp32 -> the mode's 16-bit format -> fp32."""
    assert r.dtype == torch.float32
    if mode == "fp16":
        h = r.to(torch.float16)
        if truncate:    # step the magnitude back where rounding went away from zero
            over = h.float().abs() > r.abs()
            h = torch.where(over, h.view(torch.int16) - 1, h.view(torch.int16)).view(torch.float16)
        return h.float()
    if truncate:
        return (r.contiguous().view(torch.int32) & -65536).view(torch.float32)
    return r.to(torch.bfloat16).float()


def split(x32: torch.Tensor, mode: str, truncate: bool = False, weights: bool = False, clamp: bool = True) -> List[torch.Tensor]:
    """The parts of an fp32 tensor as float64 tensors (each holds 16-bit values exactly).  ``weights``: the host packers' conversion (no clamp)."""
    assert x32.dtype == torch.float32, x32.dtype
    r = x32
    if mode == "fp16" and not weights and clamp:
        r = r.clamp(-F16_MAX, F16_MAX)
    parts = []
    for _ in range(NPARTS[mode]):
        p = _to16(r, mode, truncate)
        parts.append(p.double())
        r = r - p                      # exact in fp32, as in the kernel
    return parts


def _pairs(mode: str, mut: Mut):
    return [(_PART[t[0]], _PART[t[1]]) for t in TERMS[mode] if t != mut.drop_term]


def _terms_conv(fn, xparts, wparts, pairs, wdim, bias, acc, termwise=False, **kw):
    """sum over the terms of fn(activation part, weight part): one convolution over the terms stacked along the input channels."""
    if termwise:
        out = None
        for a, b in reversed(pairs):
            t = fn(xparts[a].flip(1).to(acc), wparts[b].flip(wdim).to(acc), None, **kw)
            out = t if out is None else out + t
        return out + bias.to(acc).reshape(1, -1, 1, 1)
    x = torch.cat([xparts[a] for a, _ in pairs], 1).to(acc)
    w = torch.cat([wparts[b] for _, b in pairs], wdim).to(acc)
    return fn(x, w, bias.to(acc), **kw)


def act32(h32: torch.Tensor, act: str, slope) -> torch.Tensor:
    """The epilogue of k_dc_x16 in fp32: max(x, slope * x) for slope <= 1, min(x, slope * x) above."""
    assert h32.dtype == torch.float32
    if act not in PWL:       # (Mut.smooth16 only: the kernels have no such instance)
        return O.activation(h32, act, None)
    s = {"relu": 0.0, "leakyrelu": 0.01}.get(act)
    s = torch.tensor(s, dtype=torch.float32) if s is not None else slope.float().reshape(())
    return torch.where(h32 >= 0, h32, h32 * s)


def q_double_conv(x, w, prefix, act, mode, acc=torch.float64, mut: Mut = SPEC):
    """The 16-bit DoubleConv on an fp32-valued input; weights fp32 tensors.  Returns dtype ``acc``."""
    p = prefix + ".double_conv."
    pairs = _pairs(mode, mut)
    xp = split(x.float(), mode, mut.truncate, clamp=not mut.no_clamp)
    h = _terms_conv(F.conv2d, xp, split(w[p + "0.weight"].float(), mode, weights=True), pairs, 1, w[p + "0.bias"], acc, mut.termwise, padding=1)
    a = act32(h.float(), act, w.get(p + "1.weight"))
    if mut.raw_mid:
        mp = [a.double()] + [torch.zeros_like(a, dtype=torch.float64)] * (NPARTS[mode] - 1)
    else:
        mp = split(a, mode, mut.truncate, clamp=not mut.no_clamp)
    w2 = split(w[p + "2.weight"].float(), mode, weights=True)
    out = _terms_conv(F.conv2d, mp, w2, pairs, 1, w[p + "2.bias"], acc, mut.termwise, padding=1)
    if mut.drop_halo:
        right = [t.clone() for t in w2]
        for t in right:
            t[..., :2] = 0
        lost = _terms_conv(F.conv2d, mp, right, pairs, 1, torch.zeros_like(w[p + "2.bias"]), acc, padding=1)
        out[..., 63::64] -= lost[..., 63::64]
    return out


def q_conv8(x, weight, bias, mode, up: bool, acc=torch.float64, mut: Mut = SPEC):
    """The 16-bit 8x8 stride-2 convolution (``up``: the transposed one), pad 3."""
    pairs = _pairs(mode, mut)
    xp, wp = split(x.float(), mode, mut.truncate, clamp=not mut.no_clamp), split(weight.float(), mode, weights=True)
    if up:
        return _terms_conv(F.conv_transpose2d, xp, wp, pairs, 0, bias, acc, mut.termwise, stride=2, padding=3)
    return _terms_conv(F.conv2d, xp, wp, pairs, 1, bias, acc, mut.termwise, stride=2, padding=3)


def quantised(layer: str, width: int, mode: Optional[str], act: str, mut: Mut = SPEC) -> bool:
    """The dispatch rule.  ``layer``: 'dc' (inc / conv_signal / bottleneck / decoder at ``width``), 'down' (``width`` = output width), 'up' (input width)."""
    if mode is None:
        return False
    if layer == "dc":
        return width >= 128 and width % 2 == 0 and (act in PWL or mut.smooth16)
    if layer == "down":
        return mode in ("fp16", "bf16x2") and width >= 64
    return width >= 64


# ------------------------------------------------------------------------------------------
# the network
# ------------------------------------------------------------------------------------------
def unet_forward(x6, states, w, depth, act="prelu", mode=None, acc=torch.float64, mut: Mut = SPEC, tape: Optional[dict] = None):
    """O.unet_forward (state_depth == depth) with the layers `quantised` names replaced by their 16-bit versions; everything in dtype ``acc``.
    ``w``: fp32 tensors.  ``tape`` receives x0, out{d}, x{d+1}, y{d}, u{d}."""
    n = x6.shape[-1]
    wa = {k: v.to(acc) for k, v in w.items()}

    def keep(name, t):
        if tape is not None:
            tape[name] = t
        return t

    def dc(x, prefix, width):
        if quantised("dc", width, mode, act, mut):
            return q_double_conv(x, w, prefix, act, mode, acc, mut)
        return O.double_conv(x.to(acc), wa, prefix, act)

    x = keep("x0", dc(x6.to(acc), "inc", n))
    skips, new_states = [], []
    for d in range(depth):
        m = n >> d
        st = states[d].to(acc)
        out = keep(f"out{d}", dc(torch.cat([x, st], 1), f"enc.{d}.conv_signal", m))
        new_states.append(O.double_conv(torch.cat([out, st], 1), wa, f"enc.{d}.conv_state", act))
        skips.append(out)
        wd, bd = f"enc.{d}.down.weight", f"enc.{d}.down.bias"
        if quantised("down", m // 2, mode, act):
            x = q_conv8(out, w[wd], w[bd], mode, False, acc, mut)
        else:
            x = F.conv2d(out, wa[wd], wa[bd], stride=2, padding=3)
        keep(f"x{d + 1}", x)
    x = keep(f"y{depth}", dc(x, f"decode.{depth}", n >> depth))
    for d in range(depth - 1, -1, -1):
        wu, bu = f"up.{d}.weight", f"up.{d}.bias"
        if quantised("up", n >> (d + 1), mode, act):
            x = q_conv8(x, w[wu], w[bu], mode, True, acc, mut)
        else:
            x = F.conv_transpose2d(x, wa[wu], wa[bu], stride=2, padding=3)
        keep(f"u{d}", x)
        x = keep(f"y{d}", dc(torch.cat([x, skips[d]], 1), f"decode.{d}", n >> d))
    return F.conv2d(x, wa["outc.conv.weight"], wa["outc.conv.bias"]), new_states


def single_step(wf, k_sq, res, states, w, source, t: O.SpectralTables, depth, act="prelu", mode=None, acc=torch.float64, mut: Mut = SPEC):
    """O.single_step around `unet_forward`.  The input layer's kernel multiplies the residual by 1e3 in fp32 while it stages it (Src::scale)."""
    sig = t.sigmas.to(acc).unsqueeze(0).repeat(wf.shape[0], 1, 1, 1)
    scaled = (res.float() * torch.tensor(1e3, dtype=torch.float32)).to(acc) if mode is not None else 1e3 * res.to(acc)
    d, new_states = unet_forward(torch.cat([wf.to(acc), scaled, sig], 1), states, w, depth, act, mode, acc, mut)
    up = d / 1e3 + wf.to(acc)
    return up, O.get_residual(up, k_sq.to(acc), source.to(acc), t), new_states


# ------------------------------------------------------------------------------------------
# layer-isolating networks
# ------------------------------------------------------------------------------------------
def passthrough_weights(depth: int, under_test: Optional[str] = None, seed: int = 771, n: int = 144) -> Dict[str, np.ndarray]:
    """A HybridNet state dict in which every layer hands its input on exactly and the layer whose names start with ``under_test`` (e.g. 'inc',
    'enc.0.conv_signal', 'enc.1.down', 'decode.0', 'up.0') has the seeded random weights of config_weights (plan A).

      DoubleConv   centre tap 1 on channel c -> c (conv_signal drops the state, a decoder passes the upsampled half), PReLU slope 1, zero bias
      down         the single tap (3, 3): out[Y, X] = in[2 Y, 2 X]
      up           the four taps {3, 4} x {3, 4} = 1: nearest-neighbour upsampling
      conv_state   centre-tap projection of the 8 features onto 2 channels, coefficients in +-[0.5, 1] (an fp32 layer in every mode)
      outc         the same projection as a 1x1 convolution
    """
    rnd = config_weights(depth, seed, "A", n=n)
    rng = np.random.default_rng(seed + 1)
    out = {}
    for name, shape in weight_shapes(depth).items():
        if under_test is not None and (name == under_test or name.startswith(under_test + ".")):
            out[name] = rnd[name]
            continue
        v = np.zeros(shape, np.float32)
        if name.endswith(".double_conv.1.weight"):
            v[:] = 1.0
        elif name.endswith(".conv_state.double_conv.0.weight") or name == "outc.conv.weight":
            coef = (rng.uniform(0.5, 1.0, (2, 8)) * rng.choice([-1.0, 1.0], (2, 8))).astype(np.float32)
            v[:, :8, shape[2] // 2, shape[3] // 2] = coef
        elif name.endswith(".double_conv.0.weight") or name.endswith(".double_conv.2.weight"):
            for c in range(min(shape[0], shape[1])):
                v[c, c, 1, 1] = 1.0
        elif name.endswith(".down.weight"):
            for c in range(8):
                v[c, c, 3, 3] = 1.0
        elif name.startswith("up.") and name.endswith(".weight"):
            for c in range(8):
                v[c, c, 3:5, 3:5] = 1.0
        out[name] = v
    return out


def exact_input(n: int, b: int, depth: int, seed: int):
    """config_input's tensors with values fp16 represents exactly: x6 and the states multiples of 2^-9 in [-2, 2]; for the step path wf = 0 and
    res = m * 2^-9 with |m| <= 16, so that 1e3 * res = 125 m * 2^-6 is exact in fp32 and in fp16."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    L = sum((n >> d) ** 2 for d in range(depth))
    sig = O.SpectralTables(n, 8, 2, 1.0).sigmas.numpy()
    wf = np.zeros((b, 2, n, n), f32)
    res = (rng.integers(-16, 17, (b, 2, n, n)) / 512.0).astype(f32)
    states = (rng.integers(-1024, 1025, (b, 2, L)) / 512.0).astype(f32)
    x6 = np.concatenate([(rng.integers(-1024, 1025, (b, 4, n, n)) / 512.0).astype(f32), np.broadcast_to(sig, (b, 2, n, n))], 1).astype(f32)
    sos = (1.0 + rng.random((b, 1, n, n))).astype(f32)
    return {"wf": wf, "res": res, "states": states, "sos": sos, "x6": np.ascontiguousarray(x6)}


# tag -> (n, depth, layer under test, 'unet' (hn_unet: d and the new states) or 'step' (hn_step: the wavefield and the new states), modes, views).
# The acceptance rule is applied to the VIEWS, the outputs that show the layer under test; every other output of the run has passed through exact layers and
# fp32 projections only and is held to the fp32 parity bar.
# Direct views (the layer's fp32 output through an fp32 projection): conv_signal_d through conv_state_d in state d; decode_0 through outc in d / the
# wavefield; down_0 of a depth-2 net through level 1 (72 wide: fp32) in state 1.  Re-rounded views (through one 16-bit pass-through, which shows the output
# rounded to the format): inc through conv_signal_0 in state 0 and d; the bottleneck, decode_1, down_1, up_0, up_1 through the 16-bit layers behind them in d.
# 144: level 0 has a partial 64-column tile, down_0 / up_0 at 72 partial 16-wide tiles; 272: level 1 is 136 wide; 256 depth 1: the 16-bit bottleneck.
_LOW = ("fp16", "bf16x2")       # k_down_x16 has no bf16x3 instance: in that mode `down` stays on the fp32 kernel (down0_144_d2 runs it as the dispatch case)
CASES = {
    "inc_144": (144, 1, "inc", "unet", MODES, ("state0", "d")),
    "sig0_144": (144, 1, "enc.0.conv_signal", "unet", MODES, ("state0", "d")),
    "dec0_144": (144, 1, "decode.0", "unet", MODES, ("d",)),
    "dec0_144_step": (144, 1, "decode.0", "step", MODES, ("wf",)),
    "up0_144": (144, 1, "up.0", "unet", MODES, ("d",)),
    "down0_144_d2": (144, 2, "enc.0.down", "unet", MODES, ("state1", "d")),
    "up0_144_d2": (144, 2, "up.0", "unet", MODES, ("d",)),
    "sig1_272": (272, 2, "enc.1.conv_signal", "unet", MODES, ("state1", "d")),
    "dec1_272": (272, 2, "decode.1", "unet", MODES, ("d",)),
    "down1_272": (272, 2, "enc.1.down", "unet", _LOW, ("d",)),
    "up1_272": (272, 2, "up.1", "unet", MODES, ("d",)),
    "bott_256": (256, 1, "decode.1", "unet", MODES, ("d",)),
}
# (case, mode) in which the layer under test stays on its fp32 kernel: the oracle's dispatch rule leaves it unquantised, the mutations do not touch it
DISPATCH = (("down0_144_d2", "bf16x3"),)
# the layer under test is a DoubleConv (Mut.raw_mid / drop_halo act on it)
DC_CASES = ("inc_144", "sig0_144", "dec0_144", "dec0_144_step", "sig1_272", "dec1_272", "bott_256")
BATCH = 2
# whole networks of random weights (bf16x3 only: its rounding flips are ~2^-24 and do not compound): tag -> (GPU_CONFIGS-style tuple, path)
WHOLE = {
    "d1_256": (GPU_CONFIGS["d1_256"][:6] + (BATCH,), "unet"),
    "d2_144": ((2, 744, "A", "prelu", 2, 144, BATCH), "unet"),
    "d2_144_step": ((2, 744, "A", "prelu", 2, 144, BATCH), "step"),
}
# dispatch: a gelu network in fp16 mode (DoubleConvs fp32, down_0 / up_0 16-bit)
GELU = ((1, 747, None, "gelu", 1, 144, BATCH), "unet")


def case_setup(tag):
    """-> dict(n, depth, act, path, w (numpy state dict), x (numpy inputs)).  'sig0_144_big': sig0_144 with sample 1 scaled by 2^17, beyond +-65504."""
    if tag == "sig0_144_big":
        c = case_setup("sig0_144")
        c["x"]["x6"][1, :4] *= 2.0 ** 17
        return c
    if tag in CASES:
        n, depth, under, path = CASES[tag][:4]
        return dict(n=n, depth=depth, act="prelu", path=path, w=passthrough_weights(depth, under, n=n),
                    x=exact_input(n, BATCH, depth, 5000 + n + depth))
    (depth, seed, plan, act, sd, n, b), path = GELU if tag == "gelu_144" else WHOLE[tag]
    return dict(n=n, depth=depth, act=act, path=path, w=config_weights(depth, seed, plan, act, sd, n=n),
                x=config_input(n, b, depth, 9000 + n, wf_scale=1e-6))


def run(c, mode, acc=torch.float64, mut: Mut = SPEC):
    """The case's outputs on the CPU: {'d' | 'wf', 'state0', ...} in dtype ``acc``."""
    n, depth = c["n"], c["depth"]
    w = {k: torch.from_numpy(v) for k, v in c["w"].items()}
    x = {k: torch.from_numpy(v) for k, v in c["x"].items()}
    st = O.unflatten_states(x["states"], n, depth)
    if c["path"] == "unet":
        d, st2 = unet_forward(x["x6"], st, w, depth, c["act"], mode, acc, mut)
        out = {"d": d}
    else:
        t = O.SpectralTables(n, 8, 2, 1.0, dtype=acc)
        k_sq, _ = O.get_initials(x["sos"], 1.0)
        wf, _, st2 = single_step(x["wf"], k_sq, x["res"], st, w, torch.zeros(1, 2, n, n), t, depth, c["act"], mode, acc, mut)
        out = {"wf": wf}
    out.update({f"state{d}": s for d, s in enumerate(st2)})
    return out


# ------------------------------------------------------------------------------------------
# acceptance
# ------------------------------------------------------------------------------------------
FP32_BAR = 1e-5           # the project's fp32 parity bar
FP16_FRACTION = 0.02      # fp16: at most this share of the elements beyond FP32_BAR ...
FP16_MAX_FACTOR = 2.0     # ... and none beyond this multiple of the twin's largest deviation (one flipped fp16 unit of a mid or viewed value)
BF16_FACTOR = 3.0         # bf16 modes: max error within this multiple of the twin's (another fp32 order of the same sums)


def errors(got, want):
    """|got - want| / max|want| per element (float64)."""
    return (got.detach().cpu().double() - want.double()).abs() / want.double().abs().max()


def rms_ratio(got, quant, plain):
    """rms(got - unquantised oracle) / rms(got - quantised oracle): how much closer ``got`` is to the 16-bit specification."""
    g = got.detach().cpu().double()
    return ((g - plain.double()).pow(2).mean().sqrt() / (g - quant.double()).pow(2).mean().sqrt().clamp_min(1e-300)).item()


def accept(mode, got, want, twin):
    """The rule for one output tensor: ``want`` the float64 oracle, ``twin`` the fp32-accumulating twin.  -> (ok, figures)."""
    e, et = errors(got, want), errors(twin, want)
    fig = {"max": e.max().item(), "twin_max": et.max().item()}
    if mode == "fp16":
        fig["over"] = (e > FP32_BAR).double().mean().item()
        fig["twin_over"] = (et > FP32_BAR).double().mean().item()
        ok = fig["over"] <= FP16_FRACTION and fig["max"] <= FP16_MAX_FACTOR * fig["twin_max"]
    else:
        ok = fig["max"] <= BF16_FACTOR * fig["twin_max"]
    return ok, fig
