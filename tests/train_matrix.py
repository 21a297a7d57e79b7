"""The training (hn_train_grad) and reverse-mode (hn_step_vjp) kernels against float64 autograd of the CPU oracle, tensor by tensor, for any
depth, activation, ``state_depth`` and weights: what ``_one_step_case`` of tests/test_training_gpu.py was for the shipped network, shared by
tests/test_train_matrix_gpu.py (HIP against float64) and tests/test_train_matrix_host.py (the fp32 oracle against float64: the bars hold for
any correct fp32 implementation; seeded errors fail them; the case list covers the dispatch).

One case goes through two legs on the same inputs and ONE oracle graph (one forward pass, two backward passes):
  (a) hn_train_grad, one unrolled iteration: loss = 1e4 * mean(res_1^2)
  (b) hn_step_vjp over that iteration: loss = <c_wf, wf_1> + <c_res, res_1> + <c_st, states_1> with seeded cotangents
Where the activation has a kink the oracle graph is evaluated AT the HIP path's pre-activation tensors (``O._keep``: straight-through), so a
pre-activation within fp32 rounding of zero takes the same branch in both.  Forcing is for what lies behind a mid; the mid itself is compared
with what the float64 graph computed at that place from the forced tensors upstream (``tape["__computed__"]``), at the forward bar like every
other forward tensor: a first convolution that is wrong is not hidden by its own output being the oracle's input.

Bars (measured against the oracle, never against the kernels): forward tensors 1e-5 * max; every gradient tensor L_inf <= 1e-4 * max of the
float64 value, or 2 x the fp32 oracle's own distance from float64 where that exceeds 5e-5 (``bars``).  A PReLU slope's gradient -- one number,
a sum of ~10^5 products of both signs -- is measured on the scale of the whole gradient.

``train_routes`` restates the dispatch of hn_train.hip (Trainer::dc_fwd, dc_bwd, merged_state and the hidden-state launches) in Python; the
training kernels carry no profile names, so "this row ran that kernel" is this function's word plus a change of bits between option values.
"""
import os
import re

import numpy as np
import torch

from config_weights import TRAIN_CONFIGS, TRAIN_INPUT_SEED, config_input, config_weights
from helmnet_amd.engine import pack_weights, unpack_weights
from oracle import helmnet_oracle as O

DEV = "cuda:0"
KINKED = ("prelu", "relu", "leakyrelu", "celu")
GEN_ACTS = ("celu", "tanh", "gelu", "tanhshrink", "softplus")      # act > HN_ACT_LEAKYRELU: the GEN instances of the kernels
PEEK_MIDS = {"sig_mid": "enc.{d}.conv_signal.mid", "st_mid": "enc.{d}.conv_state.mid", "dec_mid": "decode.{d}.mid"}
PEEK_OUTS = {"x": "x{d}", "out": "out{d}", "u": "u{d}", "y": "y{d}"}
FWD_BAR, GRAD_BAR = 1e-5, 1e-4

# the rows of tests/test_train_matrix_gpu.py (tags of config_weights.TRAIN_CONFIGS)
MATRIX = ["d4_528", "d4_80_A", "d4_80_B", "d1_80", "d2_112", "d3_144", "d5_96", "d6_192", "d6_64", "d5_160_sd2", "d4_64_sd0", "d4_80_relu",
          "d4_64_tanhshrink"]
# HN_OPT_TRAIN_FUSED values per network (55 is the default; on the first two it is the matrix row above)
ROUTE_VALUES = {"d4_80_A": (0, 1, 3, 7, 23, 55), "d4_528": (0, 7, 55), "d4_64_gelu": (0, 7, 23, 55), "d4_160_A": (0, 1, 3, 7, 23, 55)}


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def report(errs, bar):
    bad = {k: v for k, v in errs.items() if not v <= bar}
    assert not bad, f"above {bar}: {bad}\nall: {errs}"


def bars(ora, base=GRAD_BAR):
    """Per tensor: ``base``, or twice the fp32 oracle's own distance from float64 where that distance is above base / 2."""
    return {k: base if v <= base / 2 else 2 * v for k, v in ora.items()}


def worst_ratio(errs, bar):
    """(largest error / bar, its key); asserts nothing."""
    k = max(errs, key=lambda k_: errs[k_] / bar[k_])
    return errs[k] / bar[k], k


def cotangents(K, b, n, L, seed):
    """The seeded cotangents of tests/test_autograd_gpu.py (``_cot``): the residual's 1e3 times the others'."""
    g = torch.Generator().manual_seed(seed)
    return {"wf": torch.randn(K, b, 2, n, n, generator=g), "res": 1e3 * torch.randn(K, b, 2, n, n, generator=g),
            "st": torch.randn(K, b, 2, L, generator=g)}


def stateful_len(n, state_depth):
    return sum((n >> d) ** 2 for d in range(state_depth))


def make_case(depth, act, state_depth, n, b, weights, wf, res, st, sos, location=None):
    """A case from float32 tensors; the slots of the levels without state are zeroed (what the kernels are given: HybridNet.to_engine_states)."""
    location = [n // 3, n // 2] if location is None else location
    st = st.clone()
    st[:, :, stateful_len(n, state_depth):] = 0
    return dict(depth=depth, act=act, sd=state_depth, n=n, b=b, w={k: torch.as_tensor(v) for k, v in weights.items()}, wf=wf, res=res, st=st,
                k_sq=(1.0 / sos) ** 2, src=O.point_source_map(n, location, 10.0), L=st.shape[-1], La=stateful_len(n, state_depth))


def train_case(tag):
    """TRAIN_CONFIGS[tag] with its seeded weights and inputs."""
    depth, seed, plan, act, sd, n, b = TRAIN_CONFIGS[tag]
    x = config_input(n, b, depth, TRAIN_INPUT_SEED + n)
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    return make_case(depth, act, sd, n, b, config_weights(depth, seed, plan, act, sd, n=n), t["wf"], t["res"], t["states"], t["sos"])


# ---- the oracle: one graph, both legs ---------------------------------------------------------------------------------------------
def _split(case, grads, names, tkeys):
    """autograd.grad's flat tuple -> {"in": ..., "w": ..., "tape": ...}"""
    ins = dict(zip(("wf", "res", "st", "k_sq", "src"), grads[:5]))
    w = dict(zip(names, grads[5:5 + len(names)]))
    tape = dict(zip(tkeys, grads[5 + len(names):]))
    return {"in": ins, "w": w, "tape": tape}


def oracle_legs(case, dtype=torch.float64, force=None, cot=None, n_unroll=1):
    """O.training_loss in ``dtype`` (forced to the mids ``force`` if given) and its gradients.  Returns the forward tensors ("fwd": the tape
    of iteration 0 -- a forced mid as the graph computed it BEFORE the forced value took its place --, wf1 / res1 / st1, the loss), leg (a)'s gradients ("a") and, with ``cot``, leg (b)'s ("b"): each {"in", "w", "tape"},
    None where a tensor has no gradient."""
    depth, act, sd, n = case["depth"], case["act"], case["sd"], case["n"]
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=dtype)
    w = {k: v.clone().to(dtype).requires_grad_(True) for k, v in case["w"].items()}
    wf, res, st, k_sq, src = (case[k].clone().to(dtype).requires_grad_(True) for k in ("wf", "res", "st", "k_sq", "src"))
    tape = {"__stateless__": True}
    if force is not None:
        tape["__force__"], tape["__computed__"] = force, {}
    loss, wfs, ress, sts = O.training_loss(wf, res, st, k_sq, src, w, t, n_unroll, depth=depth, act=act, tape=tape, state_depth=sd)
    names = list(w)
    tkeys = [k for k in tape if not k.startswith("__")]
    inputs = [wf, res, st, k_sq, src] + [w[k] for k in names] + [tape[k] for k in tkeys]
    out = {"fwd": {k: tape[k].detach() for k in tkeys}, "loss": float(loss.detach())}
    # a forced mid's forward value is what THIS graph computed there from the forced tensors upstream (teacher-forced layer by layer): the tensor
    # the forcing implementation's own mid is compared with.  (Gradients are taken at the forced value.)
    out["fwd"].update(tape.get("__computed__", {}))
    out["fwd"].update(wf1=wfs[0].detach(), res1=ress[0].detach(), st1=sts[0].detach())
    out["a"] = _split(case, torch.autograd.grad(loss, inputs, retain_graph=cot is not None, allow_unused=True), names, tkeys)
    if cot is not None:
        loss_b = sum((cot[k][i].to(dtype) * h[i]).sum() for k, h in (("wf", wfs), ("res", ress), ("st", sts)) for i in range(n_unroll))
        out["b"] = _split(case, torch.autograd.grad(loss_b, inputs, allow_unused=True), names, tkeys)
    return out


# ---- comparison: the same function for HIP against float64 and for the fp32 oracle against float64 -------------------------------------
def _weight_errors(case, got, want, strict, tag):
    """Every weight tensor's gradient.  ``want[k] is None`` (conv_state after ONE iteration of leg (a)): structurally zero, asserted."""
    errs = {}
    have = [v for v in want.values() if v is not None]
    gmax = max(float(v.abs().max()) for v in have)
    for k, v in want.items():
        g = got[k]
        if v is None:     # conv_state feeds only the NEXT iteration: no gradient after one unrolled iteration
            assert ".conv_state." in k, k
            if strict:
                assert g is None or float(g.abs().max()) == 0.0, k
        elif v.numel() == 1:
            # a PReLU slope: ONE number, the sum of ~10^5..10^6 products of both signs; measured against the scale of the whole
            # gradient (against its own, possibly cancelled, value it is ill-conditioned in fp32 for either implementation)
            errs[tag + k] = abs(float(g.reshape(-1)[0]) - float(v)) / gmax
        else:
            errs[tag + k] = rel(g, v)
    return errs


def expected_keys(case):
    """(forward tensors, activation gradients) one iteration must be compared on: 2 * depth + 2 + state_depth mids, x / y at depth + 1 levels,
    out / u at depth levels, and wf1 / res1 / st1."""
    depth, sd = case["depth"], case["sd"]
    acts = [f"{k}{d}" for d in range(depth + 1) for k in ("x", "y")] + [f"{k}{d}" for d in range(depth) for k in ("out", "u")]
    mids = ["inc.mid"] + [f"decode.{d}.mid" for d in range(depth + 1)] + [f"enc.{d}.conv_signal.mid" for d in range(depth)] + \
           [f"enc.{d}.conv_state.mid" for d in range(sd)]
    return set(acts + mids + ["wf1", "res1"] + (["st1"] if case["La"] else [])), {"g_" + k for k in acts}


def compare(case, got, want, strict=True, whole_tape=True):
    """Errors of ``got`` (a result in oracle_legs' layout: HIP's or the fp32 oracle's) against the float64 ``want``: three dicts (forward, leg a, leg b).
    ``strict`` (HIP): what is structurally zero is asserted to be exactly zero.  ``whole_tape``: a tensor missing on either side is an error, and
    the compared keys are exactly ``expected_keys`` (off only where the caller has outputs and weight gradients alone)."""
    La, L = case["La"], case["L"]
    fwd = {k: rel(got["fwd"][k], v) for k, v in want["fwd"].items() if (whole_tape or k in got["fwd"]) and k != "st1"}
    if La:
        fwd["st1"] = rel(got["fwd"]["st1"][:, :, :La], want["fwd"]["st1"][:, :, :La])
    out = [fwd]
    for leg in ("a", "b"):
        if leg not in want:
            out.append({})
            continue
        g, w = got[leg], want[leg]
        errs = {}
        if leg == "a":
            for k, v in w["tape"].items():     # activation gradients g_x / g_out / g_u / g_y (the mids' are not peeked)
                if not k.endswith(".mid") and (whole_tape or k in g["tape"]):
                    errs["g_" + k] = rel(g["tape"][k], v)
            assert not whole_tape or (set(fwd) == expected_keys(case)[0] and {k for k in errs if k.startswith("g_")} == expected_keys(case)[1]), \
                (sorted(set(fwd) ^ expected_keys(case)[0]), sorted({k for k in errs if k.startswith("g_")} ^ expected_keys(case)[1]))
        for k in ("wf", "res", "k_sq", "src") if leg == "b" else ("wf", "res"):
            errs[f"{leg}:grad_{k}"] = rel(g["in"][k], w["in"][k])
        if La:
            errs[f"{leg}:grad_states"] = rel(g["in"]["st"][:, :, :La], w["in"]["st"][:, :, :La])
        if strict and La < L:     # the slots of the levels without state: zero weights in front of and behind them in the kernels
            assert float(g["in"]["st"][:, :, La:].abs().max()) == 0.0, leg
        if strict and leg == "a" and La == 0:
            assert w["in"]["st"] is None
        errs.update(_weight_errors(case, g["w"], w["w"], strict, leg + ":"))
        out.append(errs)
    return out


# ---- the HIP side -----------------------------------------------------------------------------------------------------------------------
def _named_grads(case, flat):
    """The flat gradient blob -> the oracle's names and shapes (the zero-padded input channels of a stateless level cut off, its
    conv_state left out)."""
    got, out = unpack_weights(flat.detach().cpu(), case["depth"]), {}
    for k, v in case["w"].items():
        g = torch.as_tensor(got[k])
        out[k] = g[:, : v.shape[1]] if g.dim() == 4 and g.shape[1] != v.shape[1] else g
    if case["act"] != "prelu":
        assert all(float(np.abs(got[k]).max()) == 0.0 for k in got if k.endswith("double_conv.1.weight"))
    return out


def _peek_all(eng, case, kinds):
    depth, b, out = case["depth"], case["b"], {}
    for kind, pat in kinds.items():
        for d in range(depth + 1):
            if d < depth or kind in ("dec_mid", "x", "y", "g_x", "g_y"):
                out[pat.format(d=d)] = eng.train_peek(kind, d, b).cpu()
    return out


def hip_mids(eng, case):
    mids = {"inc.mid": eng.train_peek("inc_mid", 0, case["b"]).cpu()}
    mids.update(_peek_all(eng, case, PEEK_MIDS))
    return mids


def hip_leg_a(eng, case):
    """hn_train_grad, one unrolled iteration, and every hn_train_peek tensor: (result in oracle_legs' layout, the mids, the call's raw output)."""
    depth, act, sd = case["depth"], case["act"], case["sd"]
    d = lambda x: x.to(DEV).contiguous()  # noqa: E731
    blob = torch.from_numpy(pack_weights({k: v.detach() for k, v in case["w"].items()}, depth, act, sd)).to(DEV)
    out = eng.train_grad(blob, d(case["wf"]), d(case["res"]), d(case["st"]), d(case["k_sq"]), d(case["src"]), 1, 1e4, input_grads=True)
    torch.cuda.synchronize()
    mids = hip_mids(eng, case)
    fwd = dict(mids)
    fwd.update(_peek_all(eng, case, PEEK_OUTS))
    fwd.update(wf1=out["wavefields"][0].cpu(), res1=out["residuals"][0].cpu(), st1=out["states"][0].cpu())
    tape = _peek_all(eng, case, {"g_" + k: v for k, v in PEEK_OUTS.items()})
    res = {"fwd": fwd, "loss": float(out["loss"][0]),
           "a": {"in": {"wf": out["grad_wf"].cpu(), "res": out["grad_res"].cpu(), "st": out["grad_states"].cpu()}, "w": _named_grads(case, out["grad"]), "tape": tape}}
    return res, mids, out, blob


def hip_leg_b(eng, case, blob, out_a, cot):
    """hn_step_vjp over the same iteration (its tape is recomputed by Trainer::forward_step from the inputs; leg (a)'s histories, which that
    function wrote, are the caller's histories) with cotangents on all three outputs."""
    d = lambda x: x.float().to(DEV).contiguous()  # noqa: E731
    k_sq = d(case["k_sq"])
    g_k, g_s, g_w = torch.zeros_like(k_sq), torch.zeros(1, 2, case["n"], case["n"], device=DEV), torch.zeros_like(blob)
    o = eng.step_vjp(blob, d(case["wf"]), d(case["res"]), d(case["st"]), k_sq, 1, out_a["wavefields"], out_a["residuals"], out_a["states"],
                     d(cot["wf"]), d(cot["res"]), d(cot["st"]), g_k_sq=g_k, g_src=g_s, g_weights=g_w)
    torch.cuda.synchronize()
    return {"in": {"wf": o["grad_wf"].cpu(), "res": o["grad_res"].cpu(), "st": o["grad_states"].cpu(), "k_sq": g_k.cpu(), "src": g_s.cpu()},
            "w": _named_grads(case, g_w), "tape": {}}


def run_case(eng, case, force_mids, leg_b=True, fp32_bars=True, cot_seed=None):
    """Both legs of one case on the engine ``eng`` (already holding the case's network and domain).  Asserts the forward bar, the loss and what is
    structurally zero; returns {"a": (errors, bars), "b": (errors, bars), "hip": the HIP results} for the caller to assert the gradient bars on."""
    n, b = case["n"], case["b"]
    got, mids, raw, blob = hip_leg_a(eng, case)
    cot = cotangents(1, b, n, case["L"], n if cot_seed is None else cot_seed) if leg_b else None
    if leg_b:
        got["b"] = hip_leg_b(eng, case, blob, raw, cot)
        again = hip_mids(eng, case)       # the recomputed forward of hn_step_vjp is Trainer::forward_step: leg (a)'s mids, bit for bit
        assert all(torch.equal(again[k], mids[k]) for k in mids), [k for k in mids if not torch.equal(again[k], mids[k])]
    eng.check_async_errors()
    force = mids if force_mids else None
    want = oracle_legs(case, torch.float64, force, cot)
    fwd, ea, eb = compare(case, got, want)
    report(fwd, FWD_BAR)       # the mids included: forced or not, HIP's own against what float64 computes there
    assert abs(got["loss"] - want["loss"]) <= 1e-5 * want["loss"]
    if fp32_bars:
        _, oa, ob = compare(case, oracle_legs(case, torch.float32, force, cot), want, strict=False)
        ba, bb = bars(oa), bars(ob)
    else:
        ba, bb = {k: GRAD_BAR for k in ea}, {k: GRAD_BAR for k in eb}
    return {"a": (ea, ba), "b": (eb, bb), "fwd": fwd, "hip": got, "raw": raw}


def assert_bars(tag, result):
    """Prints the worst error / bar of either leg and of the forward tape, then asserts every tensor's bar; returns the worst ratio."""
    worst, bad = 0.0, {}
    for leg in ("a", "b"):
        errs, bar = result[leg]
        if not errs:
            continue
        r, k = worst_ratio(errs, bar)
        worst = max(worst, r)
        print(f"[{tag}] leg ({leg}): {len(errs)} tensors, worst {errs[k]:.2e} = {r:.2f} x bar ({bar[k]:.2e}) at {k}")
        bad.update({k_: (v, bar[k_]) for k_, v in errs.items() if not v <= bar[k_]})
    f = max(result["fwd"].values()) / FWD_BAR
    print(f"[{tag}] forward tape: worst {f:.2f} x bar; WORST {max(worst, f):.2f}")
    assert not bad, f"(error, bar): {bad}"
    return worst


# ---- the dispatch of hn_train.hip, restated ----------------------------------------------------------------------------------------------
K_SMALL_S = 32          # kSmallS: a level at most this wide runs k_dc_small (one block per sample)
K_C3TW, K_C3TH = 32, 16  # kC3TW x kC3TH: tile of k_conv3 / k_dc_bwd_tile / k_dc_state_batch
K_WG_TH = 8             # kWgTH: rows of a k_conv3_wgrad tile (32 columns)
K_PART_ROWS = 640       # kPartRows: the most blocks one weight-gradient job uses; beyond it a block walks several tiles


def dc8_applies(side):
    """dc8_tape_applies / dc8_bwd_applies (hn_mfma.hip): the matrix-core DoubleConvs take even widths only."""
    return side % 2 == 0 and side > 0


def _cdiv(a, b):
    return -(-a // b)


def train_routes(n, depth, batch, fused=55):
    """Which kernel family each layer of one hn_train_grad / hn_step_vjp iteration runs on: {"fwd:inc": ..., "bwd:dec3": ..., "fwd:state": ...,
    "tiles": per-level tile facts}.  Layers: inc, sig{d} (conv_signal), dec{d} (decode; dec{depth} is the bottleneck), state (conv_state of every
    level, one dispatch).  Restated: the option bits, the parity rule, kSmallS and the channel counts.  NOT restated, because they hold for every call
    the Trainer makes today: dc8_bwd_tiles <= slope_stride (slope_stride counts the finest tiling, 8 x 16, at level 0), f3 / fb != nullptr (every
    DoubleConv of forward_step / backward_step passes its fragments), out.scale == 1 and !out.accum, in[.].act == 0, g_out.act == 0 and g_out.scale == 1
    (every caller passes plain feature tensors).  ``source_constants`` pins the TEXT of those conditions, so an edit to any of them fails the host test and
    sends its author here."""
    f_fwd, f_bwd, f_state, f_tsmall, f_mfma, f_merge = (bool(fused & m) for m in (1, 2, 4, 8, 16, 32))
    side = lambda d: n >> d  # noqa: E731
    merged = f_merge and f_mfma and f_state and all(dc8_applies(side(d)) for d in range(depth))
    layers = [("inc", 0, 6)] + [(f"sig{d}", d, 10) for d in range(depth)] + [(f"dec{d}", d, 16) for d in range(depth)] + [(f"dec{depth}", depth, 8)]
    r = {}
    for name, d, cin in layers:
        s = side(d)
        r["fwd:" + name] = "dc8_tape" if f_fwd and dc8_applies(s) else "dc_small" if s <= K_SMALL_S else "conv3_pair"
        if merged and name.startswith("dec") and d < depth:
            r["bwd:" + name] = "dc8_bwd_aux"
        elif f_mfma and dc8_applies(s):
            r["bwd:" + name] = "dc8_bwd"
        elif not f_tsmall and s <= K_SMALL_S and cin in (8, 10, 16):
            r["bwd:" + name] = "dc_small"
        else:
            r["bwd:" + name] = "dc_bwd_tile" if f_bwd else "conv3_pair"
    r["fwd:state"] = "dc_state_batch" if f_state else "conv3_batch"
    r["bwd:state"] = "dc8_bwd_aux" if merged else "dc_state_batch" if f_state else "conv3_batch"
    tiles = {}
    for d in range(depth + 1):
        s = side(d)
        wg = _cdiv(s, 32) * _cdiv(s, K_WG_TH) * batch
        tiles[d] = {"side": s, "c3_partial": s % K_C3TW != 0 or s % K_C3TH != 0, "wg_partial_cols": s % 32, "wg_partial_rows": s % K_WG_TH,
                    "wg_walks": wg > K_PART_ROWS, "wg8_partial": d > 0 and (s % 16 != 0 or s % 8 != 0)}
    r["tiles"] = tiles
    return r


def route_families(n, depth, batch, fused, act):
    """{(direction:family, GEN)} of one row."""
    r = train_routes(n, depth, batch, fused)
    return {(k.split(":")[0] + ":" + v, act in GEN_ACTS) for k, v in r.items() if k != "tiles"}


def source_constants():
    """The constants train_routes assumes, read out of the kernels' source text."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "helmnet_amd", "csrc")
    train = open(os.path.join(src, "hn_train.hip")).read()
    mfma = open(os.path.join(src, "hn_mfma.hip")).read()
    num = lambda name: int(re.search(r"constexpr int [^;]*\b" + name + r" = (\d+)", train).group(1))  # noqa: E731
    parity = {f: re.search(r"bool " + f + r"\(int H, int W\) \{ return \(W & 1\) == 0 &&", mfma) is not None for f in ("dc8_tape_applies", "dc8_bwd_applies")}
    # the dispatch conditions train_routes restates or assumes always true, as they stand in the source (whitespace-normalised)
    flat = " ".join(train.split())
    conditions = [
        "if (fused_fwd && f3 != nullptr && dc.cm == kFeat && dc.co == kFeat && dc8_tape_applies(side(d), side(d)) && out.scale == 1.f && !out.accum && "
        "in[0].act == 0 && in[1].act == 0 && in[2].act == 0) {",
        "if (small_level(d) && dc.cm == kFeat && dc.co == kFeat) {",
        "if (mfma_bwd && fb != nullptr && dc.cm == kFeat && dc.co == kFeat && g_out.act == 0 && g_out.scale == 1.f && dc8_bwd_applies(side(d), side(d)) && "
        "dc8_bwd_tiles(side(d), side(d), B) <= (int)T().slope_stride) {",
        "if (!tile_small && small_level(d) && dc.cm == kFeat && (dc.cin == kFeat || dc.cin == kFeat + kState || dc.cin == 2 * kFeat)) {",
        "if (fused_bwd && dc.cm == kFeat && dc.co == kFeat && g_out.act == 0) {",
        "if (!(merge_state && mfma_bwd && fused_state)) return false;",
        "if (!dc8_bwd_applies(side(d), side(d)) || dc8_bwd_tiles(side(d), side(d), B) > (int)T().slope_stride) return false;",
        "bool small_level(int d) const { return side(d) <= kSmallS; }",
        "W.slope_stride = (size_t)nb * cdiv(n, 16) * cdiv(n, 8);",
        "t.fused_fwd = (ctx->opt_train_fused & 1) != 0; t.fused_bwd = (ctx->opt_train_fused & 2) != 0; t.fused_state = (ctx->opt_train_fused & 4) != 0; "
        "t.tile_small = (ctx->opt_train_fused & 8) != 0; t.mfma_bwd = (ctx->opt_train_fused & 16) != 0; t.merge_state = (ctx->opt_train_fused & 32) != 0;",
    ]
    missing = [c for c in conditions if c not in flat]
    tiling = re.search(r"dc8_bwd_shape\(int H, int W, int& tw, int& tx, int& ty\) \{ tw = W > 16 \? 32 : 16; tx = cdiv_\(W, tw\); ty = cdiv_\(H, 8\); \}", mfma) is not None
    return {"conditions_missing": missing, "bwd_tiling": tiling, "kSmallS": num("kSmallS"), "kC3TW": num("kC3TW"), "kC3TH": num("kC3TH"), "kWgTH": num("kWgTH"), "kPartRows": num("kPartRows"), "parity": parity}
