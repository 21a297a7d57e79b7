"""The case list and the bars of tests/test_train_matrix_gpu.py, checked without a GPU (tests/train_matrix.py): the fp32 oracle at forced mids
meets every bar with a factor 2 to spare, seeded errors of the kind a kernel makes fail the bars by at least 10 x, and the case list reaches
every branch of the training dispatch.  CPU only."""
import functools

import pytest
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

import train_matrix as TM
from config_weights import TRAIN_CONFIGS
from oracle import helmnet_oracle as O

F64 = torch.float64
MATRIX, ROUTE_VALUES = TM.MATRIX, TM.ROUTE_VALUES


@functools.lru_cache(maxsize=None)
def _oracles(tag):
    """(case, float64 legs, errors of the fp32 oracle forced to the float64 run's pre-activations, their bars): computed once per tag."""
    case = TM.train_case(tag)
    cot = TM.cotangents(1, case["b"], case["n"], case["L"], case["n"])
    want = TM.oracle_legs(case, F64, None, cot)
    force = {k: v for k, v in want["fwd"].items() if k.endswith(".mid")} if case["act"] in TM.KINKED else None
    errs = TM.compare(case, TM.oracle_legs(case, torch.float32, force, cot), want, strict=False)
    return case, want, errs, (TM.bars(errs[1]), TM.bars(errs[2]))


@pytest.mark.parametrize("tag", list(TRAIN_CONFIGS))
def test_fp32_oracle_meets_the_bars_with_a_factor_two_to_spare(tag):
    """Stock PyTorch fp32 at the float64 run's pre-activations: forward tensors within 5e-6 * max, every gradient tensor of both legs within
    5e-5 * max of float64 (so the bar of every tensor is the plain 1e-4); every weight tensor receives a gradient in leg (b), all but
    conv_state's in leg (a)."""
    case, want, (fwd, ea, eb), _ = _oracles(tag)
    print(f"[{tag}] fp32 oracle vs float64: forward {max(fwd.values()):.2e}, leg (a) {max(ea.values()):.2e}, leg (b) {max(eb.values()):.2e}")
    TM.report(fwd, TM.FWD_BAR / 2)
    TM.report(ea, TM.GRAD_BAR / 2)
    TM.report(eb, TM.GRAD_BAR / 2)
    assert all(v is not None and float(v.abs().max()) > 0 for v in want["b"]["w"].values())
    assert all((v is None) == (".conv_state." in k) for k, v in want["a"]["w"].items())
    neg = {k: float((v < 0).double().mean()) for k, v in want["fwd"].items() if k.endswith(".mid")}
    assert len(neg) == 2 * case["depth"] + 2 + case["sd"] and min(neg.values()) >= 0.2, neg


def test_fp32_oracle_meets_the_bars_over_two_iterations():
    """The two-iteration row (tanh, depth 5): the second iteration amplifies the first one's rounding, and stock fp32 is itself 3.1e-4 from float64
    in inc's first weight gradient (sums of 2 * 96^2 products of both signs against a 1e3-scaled residual channel; five tensors lie above 5e-5).
    Those tensors get the 2 x form of the bar; none may get a bar above 1e-3, the bar of unrolled iterations elsewhere in the suite."""
    case = TM.train_case("d5_96_tanh")
    want = TM.oracle_legs(case, F64, n_unroll=2)
    fwd, ea, _ = TM.compare(case, TM.oracle_legs(case, torch.float32, n_unroll=2), want, strict=False)
    print(f"[d5_96_tanh x 2] fp32 oracle vs float64: forward {max(fwd.values()):.2e}, gradients {max(ea.values()):.2e}")
    TM.report(fwd, TM.FWD_BAR / 2)
    TM.report(ea, 5e-4)
    assert sum(v > TM.GRAD_BAR / 2 for v in ea.values()) <= 8, ea
    assert all(v is not None for v in want["a"]["w"].values())


def _same(a, b):
    assert TM.rel(a, b) <= 1e-10, TM.rel(a, b)


def _seeded_errors(tag):
    """{error: (relative error it causes, bar of the tensor it lands in)}.  Every gradient is first recomputed from the oracle's tape with
    conv2d_weight / conv2d_input and compared with autograd's; then the same recomputation with the error in it."""
    case, want, _, (ba, bb) = _oracles(tag)
    depth, sd, act, n, b = case["depth"], case["sd"], case["act"], case["n"], case["b"]
    w = {k: v.double() for k, v in case["w"].items()}
    T, ga, gb = want["fwd"], want["a"]["tape"], want["b"]["tape"]
    out = {}

    def cut(g):      # the last image column left out
        g = g.clone()
        g[..., -1] = 0
        return g

    # the bottleneck's first 3x3 convolution: dW = corr(x_depth, g_mid)
    name = f"decode.{depth}.double_conv.0.weight"
    base = conv2d_weight(T[f"x{depth}"], w[name].shape, ga[f"decode.{depth}.mid"], padding=1)
    _same(base, want["a"]["w"][name])
    out[f"3x3 wgrad, last column of {n >> depth}"] = (TM.rel(conv2d_weight(T[f"x{depth}"], w[name].shape, cut(ga[f"decode.{depth}.mid"]), padding=1), base), ba["a:" + name])
    # the bottleneck's pre-activation itself: mid = conv1(x_depth), with the last image column of its input left out
    import torch.nn.functional as F
    pre = name.replace(".weight", "")
    mid = F.conv2d(T[f"x{depth}"], w[pre + ".weight"], w[pre + ".bias"], padding=1)
    _same(mid, T[f"decode.{depth}.mid"])
    out[f"forward mid, last input column of {n >> depth}"] = (TM.rel(F.conv2d(cut(T[f"x{depth}"]), w[pre + ".weight"], w[pre + ".bias"], padding=1), mid), TM.FWD_BAR)
    # the deepest 8x8 stride-2 convolution: dW = corr(out_{depth-1}, g_x_depth)
    name = f"enc.{depth - 1}.down.weight"
    base = conv2d_weight(T[f"out{depth - 1}"], w[name].shape, ga[f"x{depth}"], stride=2, padding=3)
    _same(base, want["a"]["w"][name])
    out[f"8x8 wgrad, last column of {n >> depth}"] = (TM.rel(conv2d_weight(T[f"out{depth - 1}"], w[name].shape, cut(ga[f"x{depth}"]), stride=2, padding=3), base), ba["a:" + name])
    if sd > 0:   # grad_states of leg (b) = conv_signal's term + conv_state's term, level by level
        sig, st = [], []
        for d in range(sd):
            m = n >> d
            for terms, layer in ((sig, "conv_signal"), (st, "conv_state")):
                g = conv2d_input((b, 10, m, m), w[f"enc.{d}.{layer}.double_conv.0.weight"], gb[f"enc.{d}.{layer}.mid"], padding=1)
                terms.append(g[:, 8:10].reshape(b, 2, -1))
        sig, st = torch.cat(sig, 2), torch.cat(st, 2)
        full = want["b"]["in"]["st"][:, :, :case["La"]]
        _same(sig + st, full)
        out["conv_signal term not added into grad_states"] = (TM.rel(st, full), bb["b:grad_states"])
    # g_out0 of leg (a) = down_0's backward-data term + the decoder's skip term (conv_state's term is zero after one iteration)
    down = conv2d_input(T["out0"].shape, w["enc.0.down.weight"], ga["x1"], stride=2, padding=3)
    skip = conv2d_input((b, 16, n, n), w["decode.0.double_conv.0.weight"], ga["decode.0.mid"], padding=1)[:, 8:16]
    _same(down + skip, ga["out0"])
    out["decoder's skip term not added into g_out"] = (TM.rel(down, ga["out0"]), ba["g_out0"])
    # inc: g_mid = conv2^T(g_x0) * act'(mid); dW1 = corr(x6, g_mid); grad_res = 1e3 * (conv1^T g_mid)[residual channels]
    t = O.SpectralTables(n, 8, 2, 1.0, dtype=F64)
    x6 = torch.cat([case["wf"].double(), 1e3 * case["res"].double(), t.sigmas.unsqueeze(0).repeat(b, 1, 1, 1)], 1)
    w1 = w["inc.double_conv.0.weight"]
    if act == "prelu":
        mid = T["inc.mid"]
        g_act = conv2d_input(mid.shape, w["inc.double_conv.2.weight"], ga["x0"], padding=1)
        a_own, a_next = w["inc.double_conv.1.weight"], w["enc.0.conv_signal.double_conv.1.weight"]
        assert float(a_own) != float(a_next)
        _same(g_act * torch.where(mid > 0, torch.ones_like(mid), a_own * torch.ones_like(mid)), ga["inc.mid"])
        base = conv2d_weight(x6, w1.shape, ga["inc.mid"], padding=1)
        _same(base, want["a"]["w"]["inc.double_conv.0.weight"])
        wrong = conv2d_weight(x6, w1.shape, g_act * torch.where(mid > 0, torch.ones_like(mid), a_next * torch.ones_like(mid)), padding=1)
        out["negative branch of inc's derivative with conv_signal_0's slope"] = (TM.rel(wrong, base), ba["a:inc.double_conv.0.weight"])
    g_x6 = conv2d_input(x6.shape, w1, ga["inc.mid"], padding=1)
    _same(1e3 * g_x6[:, 2:4], want["a"]["in"]["res"])
    out["1e3 on the residual channels missing from grad_res"] = (TM.rel(g_x6[:, 2:4], want["a"]["in"]["res"]), ba["a:grad_res"])
    return out


@pytest.mark.parametrize("tag", MATRIX + ["d4_64_gelu"])
def test_seeded_errors_fail_the_bars(tag):
    """What a kernel gets wrong when it is subtly wrong (a partial tile's last column, a term of a sum that two launches share, the wrong slot of
    the slope table, a scale) lands at least 10 x above the bar of the tensor it touches, on every case it applies to."""
    factors = {k: e / bar for k, (e, bar) in _seeded_errors(tag).items()}
    print(f"[{tag}] seeded error / bar: " + "; ".join(f"{k}: {v:.0f} x" for k, v in factors.items()))
    assert all(v >= 10 for v in factors.values()), factors


def test_the_case_list_covers_the_dispatch():
    """Over the GPU rows, train_routes reaches every branch of dc_fwd, dc_bwd and the hidden-state dispatch, each in a GEN and a non-GEN
    activation where the kernel is instantiated for both; and the constants train_routes assumes are the ones in the source."""
    c = TM.source_constants()
    assert (c["kSmallS"], c["kC3TW"], c["kC3TH"], c["kWgTH"], c["kPartRows"]) == (TM.K_SMALL_S, TM.K_C3TW, TM.K_C3TH, TM.K_WG_TH, TM.K_PART_ROWS), c
    assert c["parity"] == {"dc8_tape_applies": True, "dc8_bwd_applies": True}, c
    # the conditions of dc_fwd / dc_bwd / merged_state, the option bits and the slope-partials bound as train_routes read them: an edit to any of them
    # fails here, and train_routes is then revised with it
    assert not c["conditions_missing"] and c["bwd_tiling"], c
    for n, depth, b in {(v[5], v[0], v[6]) for v in TRAIN_CONFIGS.values()}:     # the bound train_routes leaves out: never binding
        assert all(TM._cdiv(n >> d, 32 if (n >> d) > 16 else 16) * TM._cdiv(n >> d, 8) * b <= b * TM._cdiv(n, 16) * TM._cdiv(n, 8) for d in range(depth + 1))
    rows = [(t, 55) for t in MATRIX + ["d5_96_tanh"]] + [(t, v) for t, vs in ROUTE_VALUES.items() for v in vs]
    seen = set()
    for tag, fused in rows:
        depth, _, _, act, _, n, b = TRAIN_CONFIGS[tag]
        seen |= TM.route_families(n, depth, b, fused, act)
    both = ["fwd:dc_small", "fwd:conv3_pair", "fwd:dc_state_batch", "fwd:conv3_batch", "bwd:dc_small", "bwd:dc_bwd_tile", "bwd:conv3_pair",
            "bwd:dc_state_batch", "bwd:conv3_batch"]                  # kernels with a GEN template flag
    runtime = ["fwd:dc8_tape", "bwd:dc8_bwd", "bwd:dc8_bwd_aux"]      # the matrix-core DoubleConvs take the activation as an argument
    missing = [(f, g) for f in both for g in (False, True) if (f, g) not in seen] + [f for f in runtime if not {(f, False), (f, True)} & seen]
    assert not missing, missing
    # the default fall-through: an odd bottleneck wider than kSmallS, reached by d4_528 alone
    r = TM.train_routes(528, 4, 1, 55)
    assert r["fwd:dec4"] == "conv3_pair" and r["bwd:dec4"] == "dc_bwd_tile" and r["bwd:dec3"] == "dc8_bwd_aux" and r["tiles"][4]["wg_partial_cols"] == 1
    assert all(TM.train_routes(TRAIN_CONFIGS[t][5], TRAIN_CONFIGS[t][0], TRAIN_CONFIGS[t][6], 55)["fwd:dec%d" % TRAIN_CONFIGS[t][0]] != "conv3_pair"
               for t in MATRIX if t != "d4_528")
    # every option value of a route row changes the family of at least one layer against its neighbour
    for tag, vs in ROUTE_VALUES.items():
        depth, _, _, _, _, n, b = TRAIN_CONFIGS[tag]
        for u, v in zip(vs, vs[1:]):
            ru, rv = TM.train_routes(n, depth, b, u), TM.train_routes(n, depth, b, v)
            assert any(ru[k] != rv[k] for k in ru if k != "tiles"), (tag, u, v)


def test_a_wrong_forced_mid_fails_the_forward_bar():
    """The harness as the GPU test runs it on a kinked row, the fp32 oracle standing in for the kernels: the float64 graph is forced to the stand-in's
    mids, and each of those mids is still compared with what float64 computes at its place.  The stand-in's own mids pass; the bottleneck's mid
    with its last column computed from an input without its last column (what a partial tile's edge gets wrong) fails by more than 10 x, although
    every tensor behind it is then computed FROM the wrong mid on both sides."""
    import torch.nn.functional as F
    case = TM.train_case("d4_80_A")
    got = TM.oracle_legs(case, torch.float32)
    mids = {k: v.clone() for k, v in got["fwd"].items() if k.endswith(".mid")}
    fwd, _, _ = TM.compare(case, got, TM.oracle_legs(case, F64, mids), strict=False)
    TM.report(fwd, TM.FWD_BAR / 2)
    depth, pre = case["depth"], f"decode.{case['depth']}.double_conv.0"
    x = got["fwd"][f"x{depth}"].clone()
    x[..., -1] = 0
    wrong = F.conv2d(x, case["w"][pre + ".weight"], case["w"][pre + ".bias"], padding=1)
    name = f"decode.{depth}.mid"
    mids[name] = torch.cat([mids[name][..., :-1], wrong[..., -1:]], -1)      # only the last column differs
    got["fwd"][name] = mids[name]
    fwd, _, _ = TM.compare(case, got, TM.oracle_legs(case, F64, mids), strict=False)
    print(f"wrong last column of {name}: {fwd[name] / TM.FWD_BAR:.0f} x the forward bar")
    # (the stand-in's decoder mids were computed from its own bottleneck, so only the tensors in front of the bottleneck still have to agree)
    assert fwd[name] >= 10 * TM.FWD_BAR and all(v <= TM.FWD_BAR / 2 for k, v in fwd.items() if k.endswith(".mid") and not k.startswith("decode."))
