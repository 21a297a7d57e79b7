"""The 16-bit UNet kernels (k_dc_x16<HalfF16 | SplitBf16x2 | SplitBf16>, k_down_x16, k_up_x16 of hn_mfma.hip) against the operand-rounded float64 oracle of
tests/x16_oracle.py, to fp32-accumulation accuracy instead of to the accuracy of the format.  Needs a real MI355X.

Each case is a network in which one layer has random weights and every other layer hands its input on exactly (x16_oracle.CASES), at the smallest sizes that
reach each kernel instance with partial tiles, batch 2.  The rule (x16_oracle.accept), per output that shows the layer, relative to max|oracle|:
  bf16x3, bf16x2   max error <= 3 x the largest deviation of the CPU twin (the same rounded operands summed in fp32 in another order)
  fp16             at most 2 % of the elements beyond 1e-5, and max error <= 2 x the twin's largest deviation (one flipped fp16 unit)
and, in fp16 and bf16x2, the kernel is closer in rms to the quantised oracle than to the unquantised one by at least half the ratio the twin shows: the 16-bit
kernel of that mode ran.  tests/test_x16_host.py shows on the CPU that the twin meets the rule with room and that every mutation of the arithmetic fails it.
Every test prints the twin's and the GPU's figures before it asserts.
"""
import pytest
import torch

import x16_oracle as X
from config_solver import _solver, _step, _unet
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

_REF = {}


def _refs(tag, mode, mut=X.SPEC):
    """CPU results of a case, computed once: the float64 oracle and the twin of ``mode``, the unquantised float64 oracle under mode None."""
    key = (tag, mode, mut)
    if key not in _REF:
        c = X.case_setup(tag)
        _REF[key] = X.run(c, None) if mode is None else (X.run(c, mode, mut=mut), X.run(c, mode, acc=torch.float32, mut=mut))
    return _REF[key]


def _gpu(c, mode, x=None):
    x = c["x"] if x is None else x
    s = _solver(c["depth"], c["act"], None, c["w"], c["n"], mode=mode)
    assert s.engine().unet_precision == mode
    if c["path"] == "unet":
        out = {"d": _unet(s, x).cpu()}
        flat = s.f.get_states(flatten=True).cpu()
    else:
        wf, _, flat = _step(s, x)
        out, flat = {"wf": wf.cpu()}, flat.cpu()
    s.engine().check_async_errors()
    out.update({f"state{d}": t for d, t in enumerate(O.unflatten_states(flat, c["n"], c["depth"]))})
    return out


def _check(tag, mode, got, want, twin, plain, views):
    """The acceptance rule on the views, the fp32 parity bar on every other output.  -> (failures, report lines)"""
    bad, report = [], []
    for k in want:
        ok, fig = X.accept(mode, got[k], want[k], twin[k])
        line = f"{k}: gpu max {fig['max']:.2e} (twin {fig['twin_max']:.2e})"
        if k not in views:
            ok = fig["max"] <= X.FP32_BAR
        elif mode == "fp16":
            line += f", beyond 1e-5 {fig['over']:.2%} (twin {fig['twin_over']:.2%})"
        if k in views and mode != "bf16x3" and plain is not None:
            r_gpu, r_twin = X.rms_ratio(got[k], want[k], plain[k]), X.rms_ratio(twin[k], want[k], plain[k])
            line += f", rms ratio {r_gpu:.1f} (twin {r_twin:.1f})"
            ok = ok and r_gpu >= 0.5 * r_twin
        report.append(line)
        if not ok:
            bad.append(k)
    print(f"[{tag} {mode}] " + "; ".join(report))
    return bad, report


@pytest.mark.parametrize("tag,mode", [(tag, mode) for tag, c in X.CASES.items() for mode in c[4]])
def test_one_16_bit_layer_between_exact_layers_vs_the_rounded_oracle(tag, mode):
    c = X.case_setup(tag)
    views = X.CASES[tag][5]
    (want, twin), plain = _refs(tag, mode), _refs(tag, None)
    got = _gpu(c, mode)
    bad, report = _check(tag, mode, got, want, twin, plain, views)
    assert not bad, (bad, report)
    if mode == "bf16x3" and (tag, mode) not in X.DISPATCH:     # (no rms ratio tells bf16x3 from fp32: the bits do)
        ref = _gpu(c, "fp32")
        assert any(not torch.equal(got[k], ref[k]) for k in views)


@pytest.mark.parametrize("tag", list(X.WHOLE))
def test_whole_networks_in_bf16x3_vs_the_rounded_oracle(tag):
    """Random weights in every layer (bf16x3 only: its rounding flips are ~2^-24 and do not compound): every output within 3 x the twin's deviation and within
    the fp32 parity bar."""
    c = X.case_setup(tag)
    want, twin = _refs(tag, "bf16x3")
    got = _gpu(c, "bf16x3")
    bad, report = _check(tag, "bf16x3", got, want, twin, None, tuple(want))
    assert not bad and all(float(X.errors(got[k], want[k]).max()) <= X.FP32_BAR for k in want), (bad, report)
    ref = _gpu(c, "fp32")
    assert any(not torch.equal(got[k], ref[k]) for k in want)


def test_gelu_in_fp16_mode_runs_fp32_doubleconvs_and_16_bit_down_and_up():
    """Dispatch: a smooth activation keeps the DoubleConvs on their fp32 instances in every mode, while down_0 / up_0 (72 wide) run in 16 bits.  d is closer in
    rms to the oracle of that dispatch than to the unquantised one and to the one with 16-bit DoubleConvs (half the twin's ratios, which the host test shows to
    be above 4); state 0 (conv_signal_0 and conv_state_0: fp32) meets the fp32 parity bar; the largest error is within 2 x the twin's (one flipped fp16 unit)."""
    tag = "gelu_144"
    c = X.case_setup(tag)
    (want, twin), plain = _refs(tag, "fp16"), _refs(tag, None)
    all16, _ = _refs(tag, "fp16", X.Mut(smooth16=True))
    got = _gpu(c, "fp16")
    fig = {name: (X.rms_ratio(got["d"], want["d"], other["d"]), X.rms_ratio(twin["d"], want["d"], other["d"])) for name, other in (("plain", plain), ("all16", all16))}
    e_d, t_d = float(X.errors(got["d"], want["d"]).max()), float(X.errors(twin["d"], want["d"]).max())
    e_s = float(X.errors(got["state0"], want["state0"]).max())
    print(f"[{tag} fp16] d: gpu max {e_d:.2e} (twin {t_d:.2e}), rms ratio against the unquantised oracle {fig['plain'][0]:.1f} (twin {fig['plain'][1]:.1f}), "
          f"against 16-bit DoubleConvs {fig['all16'][0]:.1f} (twin {fig['all16'][1]:.1f}); state0: gpu max {e_s:.2e}")
    assert all(g >= 0.5 * t for g, t in fig.values()), fig
    assert e_s <= X.FP32_BAR and e_d <= X.FP16_MAX_FACTOR * t_d


def test_fp16_a_sample_beyond_65504_is_clamped_and_leaves_the_other_alone():
    """sig0_144 with sample 1 scaled by 2^17: HalfF16::split saturates, so the sample's outputs are finite and equal the clamping oracle (the fp16 rule on the
    sample's own scale); sample 0 has the bits of its run alone."""
    tag = "sig0_144_big"
    c = X.case_setup(tag)
    want, twin = _refs(tag, "fp16")
    got = _gpu(c, "fp16")
    alone = _gpu(c, "fp16", {k: v[:1] for k, v in c["x"].items()})
    bad = []
    for k in ("state0", "d"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k][:1], alone[k]), k
        ok, fig = X.accept("fp16", got[k][1:], want[k][1:], twin[k][1:])
        print(f"[{tag} fp16] {k}, sample 1: max|oracle| {float(want[k][1].abs().max()):.3e}, gpu max {fig['max']:.2e} (twin {fig['twin_max']:.2e}), "
              f"beyond 1e-5 {fig['over']:.2%} (twin {fig['twin_over']:.2%})")
        if not ok:
            bad.append(k)
    assert not bad
