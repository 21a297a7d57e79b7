"""The operand-rounded oracle of the 16-bit UNet modes (tests/x16_oracle.py) and the bars of tests/test_x16_gpu.py, checked on the CPU (no GPU needed):

  * with quantisation off the oracle IS O.unet_forward / O.single_step;
  * `split` agrees, bit for bit, with the integer arithmetic of the host packers (bf16_rne / f16_rne of hn_mfma.hip, restated below) on edge values;
  * every pass-through network hands its input on exactly in the fp32-accumulating twin, in all three modes;
  * for every GPU case the twin -- a correct implementation with another summation order -- meets the acceptance rule with room to spare, and a second twin
    with yet another order meets the rule whose bars the first one sets;
  * every mutation of the arithmetic fails the rule in every mode in which it changes a value above fp32 accumulation noise, and the bf16 bars lie below half
    the deviation of the weakest single-term mutation.  This is what shows that the bars are tight enough.
"""
import numpy as np
import pytest
import torch

import x16_oracle as X
from oracle import helmnet_oracle as O

_CACHE = {}


def _runs(tag, mode):
    """(float64 oracle, twin, unquantised float64 oracle) of a case, computed once."""
    if (tag, None) not in _CACHE:
        _CACHE[(tag, None)] = X.run(X.case_setup(tag), None)
    if (tag, mode) not in _CACHE:
        c = X.case_setup(tag)
        _CACHE[(tag, mode)] = (X.run(c, mode), X.run(c, mode, acc=torch.float32))
    return _CACHE[(tag, mode)] + (_CACHE[(tag, None)],)


def test_with_quantisation_off_the_oracle_is_the_projects_oracle():
    c = X.case_setup("d2_144")
    n, depth = c["n"], c["depth"]
    for dtype in (torch.float32, torch.float64):
        w = {k: torch.from_numpy(v).to(dtype) for k, v in c["w"].items()}
        x = {k: torch.from_numpy(v).to(dtype) for k, v in c["x"].items()}
        st = O.unflatten_states(x["states"], n, depth)
        d, st2 = O.unet_forward(x["x6"], st, w, depth)
        got = X.run(c, None, acc=dtype)
        assert torch.equal(got["d"], d) and all(torch.equal(got[f"state{i}"], s) for i, s in enumerate(st2))
        t = O.SpectralTables(n, 8, 2, 1.0, dtype=dtype)
        k_sq, _ = O.get_initials(x["sos"], 1.0)
        wf, res, st3 = O.single_step(x["wf"], k_sq, x["res"], st, w, torch.zeros(1, 2, n, n, dtype=dtype), t, depth)
        wf2, res2, st4 = X.single_step(x["wf"], k_sq, x["res"], st, {k: torch.from_numpy(v) for k, v in c["w"].items()},
                                       torch.zeros(1, 2, n, n), t, depth, acc=dtype)
        assert torch.equal(wf, wf2) and torch.equal(res, res2) and all(torch.equal(a, b) for a, b in zip(st3, st4))


# ---- the host packers' conversions (hn_mfma.hip: bf16_rne, f16_rne), restated on integers ----
def _bf16_rne_bits(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_f(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def _f16_rne_bits(x):
    out = []
    for u in np.asarray(x, np.float32).view(np.uint32).tolist():
        sign, ex, man = (u >> 16) & 0x8000, (u >> 23) & 0xFF, u & 0x7FFFFF
        e = ex - 127 + 15
        if ex == 0xFF:
            out.append(sign | 0x7C00 | (0x200 if man else 0))
        elif e >= 31:
            out.append(sign | 0x7C00)
        elif e <= 0:
            if e < -10:
                out.append(sign)
                continue
            man |= 0x800000
            shift = 14 - e
            h, rem, half = man >> shift, man & ((1 << shift) - 1), 1 << (shift - 1)
            out.append(sign | (h + (rem > half or (rem == half and h & 1))))
        else:
            h, rem = (e << 10) | (man >> 13), man & 0x1FFF
            out.append(sign | (h + (rem > 0x1000 or (rem == 0x1000 and h & 1))))
    return np.array(out, np.uint16)


def _edge_values():
    f = np.float32
    v = [0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 - 2.0 ** -12,      # fp16 ties to even, both ways
         1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 + 2.0 ** -16,                    # bf16 ties; a second-part tie
         2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -25, 1e-7,      # fp16 subnormals and below
         65504.0, -65504.0, 65519.0, 65520.0, 65536.0, -1e6, 3.0e38, 1.1754944e-38, 0.1, -0.3, 3.14159265, 1e-3, 123.456]
    rng = np.random.default_rng(5)
    return np.concatenate([np.array(v, f), (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 5, 4000)).astype(f)])


def test_split_agrees_with_the_host_packers_on_edge_values():
    v = _edge_values()
    t = torch.from_numpy(v)
    # bf16: three parts, each the packer's round-to-nearest-even of the fp32 remainder (pack_k8_x16 / pack_frag_3x3_split)
    h = _bf16_rne_bits(v)
    r1 = v - _bf16_f(h)
    m = _bf16_rne_bits(r1)
    lo = _bf16_rne_bits(r1 - _bf16_f(m))
    for mode, want in (("bf16x3", (h, m, lo)), ("bf16x2", (h, m))):
        parts = X.split(t, mode)
        assert len(parts) == len(want)
        for p, bits in zip(parts, want):
            assert p.dtype == torch.float64 and np.array_equal(p.float().numpy().view(np.uint32), _bf16_f(bits).view(np.uint32)), mode
    # the three parts carry at least 24 bits: x = h + m + l exactly, away from the underflow of the last part
    big = np.abs(v) > 1e-30
    s3 = sum(X.split(t, "bf16x3")).float().numpy()
    assert np.array_equal(s3[big], v[big])
    # fp16 weights: f16_rne, saturating to infinity; fp16 activations: the same after the clamp to +-65504 (HalfF16::split)
    (pw,) = X.split(t, "fp16", weights=True)
    assert np.array_equal(pw.float().numpy().astype(np.float16).view(np.uint16), _f16_rne_bits(v))
    assert np.isinf(pw.numpy()[np.abs(v) >= 65520.0]).all()
    (pa,) = X.split(t, "fp16")
    assert np.array_equal(pa.float().numpy().astype(np.float16).view(np.uint16), _f16_rne_bits(np.clip(v, -65504.0, 65504.0)))
    assert np.isfinite(pa.numpy()).all() and float(pa.abs().max()) == 65504.0
    # truncation never rounds away from zero and differs from RNE somewhere
    for mode in X.MODES:
        tr, rn = X.split(t, mode, truncate=True)[0], X.split(t, mode)[0]
        clamped = t.clamp(-65504, 65504).double() if mode == "fp16" else t.double()
        assert bool((tr.abs() <= clamped.abs()).all()) and not torch.equal(tr, rn), mode
        assert bool(((tr - clamped).abs() < 2 * (rn - clamped).abs() + clamped.abs() * 2.0 ** -7 + 2.0 ** -24).all())


@pytest.mark.parametrize("n,depth", [(144, 1), (144, 2), (272, 2), (256, 1)])
def test_every_passthrough_network_hands_its_input_on_exactly(n, depth):
    """No layer under test: in the twin, in every mode, the feature tensors are the first four input channels and the sigmas, subsampled and repeated, bit
    for bit; the outputs are the fp32 projections of those (one rounding per product and sum: compared with the float64 oracle at fp32 accuracy)."""
    w = {k: torch.from_numpy(v) for k, v in X.passthrough_weights(depth, None, n=n).items()}
    x = {k: torch.from_numpy(v) for k, v in X.exact_input(n, X.BATCH, depth, 5000 + n + depth).items()}
    assert torch.equal(x["x6"].half().float(), x["x6"]) and torch.equal(x["states"].half().float(), x["states"])
    scaled = x["res"] * torch.tensor(1e3, dtype=torch.float32)
    assert torch.equal(scaled.double(), 1e3 * x["res"].double()) and torch.equal(scaled.half().float(), scaled)
    st = O.unflatten_states(x["states"], n, depth)
    feat = torch.cat([x["x6"], torch.zeros(X.BATCH, 2, n, n)], 1)
    want = {"x0": feat, "out0": feat}
    lvl = feat
    for d in range(depth):
        lvl = lvl[..., ::2, ::2]
        want[f"x{d + 1}"] = lvl
    want[f"y{depth}"] = lvl
    for d in range(depth - 1, -1, -1):
        lvl = lvl.repeat_interleave(2, -1).repeat_interleave(2, -2)
        want[f"u{d}"] = want[f"y{d}"] = lvl
    for d in range(1, depth):
        want[f"out{d}"] = want[f"x{d}"]
    outs = {}
    for mode in X.MODES + (None,):
        tape = {}
        d, st2 = X.unet_forward(x["x6"], st, w, depth, "prelu", mode, torch.float32, tape=tape)
        assert set(tape) == set(want)
        for k, v in want.items():
            assert torch.equal(tape[k], v), (mode, k)
        outs[mode] = [d] + st2
    d64, st64 = X.unet_forward(x["x6"], st, w, depth, "prelu", "fp16", torch.float64)
    for mode in X.MODES:
        for a, b, e in zip(outs[mode], outs[None], [d64] + st64):
            assert torch.equal(a, b) and float(X.errors(a, e).max()) <= 2e-7, mode


GPU_CASES = [(tag, mode) for tag, c in X.CASES.items() for mode in c[4]]


@pytest.mark.parametrize("tag,mode", GPU_CASES)
def test_the_twin_meets_the_rule_with_room_and_every_mutation_fails_it(tag, mode):
    want, twin, plain = _runs(tag, mode)
    views = X.CASES[tag][5]
    report = []
    for k in want:
        ok, fig = X.accept(mode, twin[k], want[k], twin[k])
        assert ok
        if k not in views:      # exact layers and fp32 projections only
            assert fig["twin_max"] <= 0.1 * X.FP32_BAR, (k, fig)
            continue
        if mode == "fp16":      # the 2 % of the rule is a condition: the twin itself stays at or below 1 % on these inputs
            assert fig["twin_over"] <= 0.5 * X.FP16_FRACTION, (k, fig)
            assert fig["twin_max"] <= 6e-4, (k, fig)     # one fp16 unit of a mid or viewed value (2^-11 relative), through weights of order 1
        else:                   # the bar 3 x twin: bf16x2 a few units of 2^-17, bf16x3 of 2^-24
            assert X.BF16_FACTOR * fig["twin_max"] <= (3e-5 if mode == "bf16x2" else 2e-6), (k, fig)
        ratio = X.rms_ratio(twin[k], want[k], plain[k])
        report.append(f"{k}: twin max {fig['twin_max']:.2e}" + (f", beyond 1e-5 {fig['twin_over']:.2%}" if mode == "fp16" else "") + f", rms ratio {ratio:.1f}")
        if mode != "bf16x3":    # the GPU test asserts half of this ratio: it must tell the 16-bit specification from the unrounded one
            assert ratio >= 2.5, (k, ratio)
    print(f"[{tag} {mode}] " + "; ".join(report))
    # a second correct implementation (one convolution per term, another channel order) meets the rule whose bars the first twin sets
    c = X.case_setup(tag)
    other = X.run(c, mode, acc=torch.float32, mut=X.Mut(termwise=True))
    for k in views:
        ok, fig = X.accept(mode, other[k], want[k], twin[k])
        print(f"    second twin {k}: max {fig['max']:.2e}" + (f", beyond 1e-5 {fig['over']:.2%}" if mode == "fp16" else ""))
        assert ok, (k, fig)
    if (tag, mode) in X.DISPATCH:
        return
    # ---- mutations ----
    muts = dict(X.term_mutations(mode))
    if mode != "bf16x3":               # (three parts carry 24 bits: the rounding mode of the last one is below fp32 accumulation noise)
        muts["truncate"] = X.MUTATIONS["truncate"]
    if tag in X.DC_CASES:
        muts["drop_halo"] = X.MUTATIONS["drop_halo"]
        if mode == "fp16":             # (bf16x2: an unrounded mid is off by half a 16-bit unit per tap, 4.7e-6 - 8.1e-6 against bars of 8.3e-6 - 1.7e-5: not detected)
            muts["raw_mid"] = X.MUTATIONS["raw_mid"]
    weakest = {k: float("inf") for k in views}
    for name, m in muts.items():
        bad = X.run(c, mode, acc=torch.float32, mut=m)
        fails = []
        for k in views:
            ok, fig = X.accept(mode, bad[k], want[k], twin[k])
            fails.append(not ok)
            if name.startswith("drop_") and name != "drop_halo":
                weakest[k] = min(weakest[k], fig["max"])
        print(f"    {name}: " + ", ".join(f"{k} {'fails' if f else 'passes'}" for k, f in zip(views, fails)))
        assert any(fails), (tag, mode, name)
        if name.startswith("drop_") and name != "drop_halo":
            assert all(fails), (tag, mode, name)      # a missing term shows in every view
    if mode != "fp16":
        for k in views:     # the bar stays at or below half the deviation of the weakest single-term mutation
            _, fig = X.accept(mode, twin[k], want[k], twin[k])
            assert X.BF16_FACTOR * fig["twin_max"] <= 0.5 * weakest[k], (k, fig, weakest[k])


@pytest.mark.parametrize("tag", list(X.WHOLE))
def test_whole_networks_in_bf16x3_the_twin_stays_below_a_third_of_the_parity_bar(tag):
    c = X.case_setup(tag)
    want, twin = X.run(c, "bf16x3"), X.run(c, "bf16x3", acc=torch.float32)
    for k in want:
        ok, fig = X.accept("bf16x3", twin[k], want[k], twin[k])
        print(f"[{tag}] {k}: twin max {fig['twin_max']:.2e}")
        assert ok and X.BF16_FACTOR * fig["twin_max"] <= X.FP32_BAR, (k, fig)
    for name, m in X.term_mutations("bf16x3").items():
        bad = X.run(c, "bf16x3", acc=torch.float32, mut=m)
        assert not all(X.accept("bf16x3", bad[k], want[k], twin[k])[0] for k in want), name


def test_the_gelu_dispatch_case_tells_the_three_dispatches_apart():
    """fp16 mode, gelu: the DoubleConvs stay in fp32, down_0 / up_0 run in 16 bits.  The twin of that dispatch is closer in rms to its oracle than to the
    unquantised one and to the one that also runs the DoubleConvs in 16 bits, by more than the factor 2 the GPU test halves."""
    c = X.case_setup("gelu_144")
    want, twin = X.run(c, "fp16"), X.run(c, "fp16", acc=torch.float32)
    plain, all16 = X.run(c, None), X.run(c, "fp16", mut=X.Mut(smooth16=True))
    r_plain, r_all16 = X.rms_ratio(twin["d"], want["d"], plain["d"]), X.rms_ratio(twin["d"], want["d"], all16["d"])
    print(f"[gelu_144 fp16] d: rms ratio against the unquantised oracle {r_plain:.1f}, against 16-bit DoubleConvs {r_all16:.1f}; "
          f"twin max {float(X.errors(twin['d'], want['d']).max()):.2e}, state0 {float(X.errors(twin['state0'], want['state0']).max()):.2e}")
    assert r_plain >= 4.0 and r_all16 >= 4.0
    assert float(X.errors(twin["state0"], want["state0"]).max()) <= 0.3 * X.FP32_BAR      # conv_signal_0 and conv_state_0 are fp32 layers here
    assert float(X.errors(all16["state0"], want["state0"]).max()) > X.FP32_BAR


def test_a_sample_beyond_the_fp16_range_is_clamped_not_infinite():
    """sig0_144 with sample 1 scaled by 2^17: the specification clamps activations (inputs and mid tensors) to +-65504, so the sample stays finite and its
    twin meets the fp16 rule on its own scale; without the clamp it is not finite."""
    c = X.case_setup("sig0_144_big")
    assert float(np.abs(c["x"]["x6"][1]).max()) > 4 * X.F16_MAX and float(np.abs(c["x"]["x6"][0]).max()) <= 2.0
    want, twin = X.run(c, "fp16"), X.run(c, "fp16", acc=torch.float32)
    base = X.run(X.case_setup("sig0_144"), "fp16")
    for k in ("state0", "d"):
        assert bool(torch.isfinite(want[k]).all()) and torch.equal(want[k][0], base[k][0])
        ok, fig = X.accept("fp16", twin[k][1:], want[k][1:], twin[k][1:])
        print(f"[sig0_144_big fp16] {k}, sample 1: max|want| {float(want[k][1].abs().max()):.3e}, twin max {fig['twin_max']:.2e}, beyond 1e-5 {fig['twin_over']:.2%}")
        assert ok and fig["twin_over"] <= 0.5 * X.FP16_FRACTION
    bad = X.run(c, "fp16", acc=torch.float32, mut=X.Mut(no_clamp=True))
    assert not bool(torch.isfinite(bad["state0"][1]).all()) and bool(torch.isfinite(bad["state0"][0]).all())
