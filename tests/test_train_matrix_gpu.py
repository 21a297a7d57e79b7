"""hn_train_grad and hn_step_vjp on every network and route against float64 autograd of the CPU oracle, tensor by tensor (the harness and the
bars: tests/train_matrix.py): depths 1 - 6, both PReLU slope plans, relu, tanhshrink, gelu, state_depth < depth, an odd bottleneck wider than 32
(528 = 16 * 33: the default fall-through of dc_fwd / dc_bwd), and every HN_OPT_TRAIN_FUSED value against float64 rather than against the default.
Needs a real MI355X: ``python -m pytest tests -m gpu``.

Measured worst error / bar per row: DESIGN.md section 7, "training routes and their tests"."""
import pytest
import torch

import train_matrix as TM
from config_solver import DEV, _solver
from config_weights import TRAIN_CONFIGS, config_weights
from helmnet_amd.engine import pack_weights

pytestmark = pytest.mark.gpu

MATRIX, ROUTE_VALUES = TM.MATRIX, TM.ROUTE_VALUES
ROUTE_ROWS = [(t, v) for t, vs in ROUTE_VALUES.items() for v in vs if not (v == 55 and t in MATRIX)]
BIT_IDENTICAL = 2 | 4          # the header's unqualified promise: bit-identical gradients
MAY_BE_IDENTICAL = 16          # ... and "bit-identical gradients at the training sizes": nothing asserted either way
NARROW = 128                   # below this width value 1 is MEASURED bit-identical to 0 (a property of today's kernels, no promise): see the test


def _promised(u, v):
    return (u ^ v) & ~BIT_IDENTICAL == 0


def _engine(tag):
    depth, seed, plan, act, sd, n, _ = TRAIN_CONFIGS[tag]
    s = _solver(depth, act, sd, config_weights(depth, seed, plan, act, sd, n=n), n)
    return s, s.engine()


def _row(tag, fused=55):
    case = TM.train_case(tag)
    s, eng = _engine(tag)
    try:
        eng.set_option("train_fused", fused)
        result = TM.run_case(eng, case, force_mids=case["act"] in TM.KINKED)
    finally:
        eng.set_option("train_fused", 55)
    label = tag if fused == 55 else f"{tag} fused {fused}"
    routes = TM.train_routes(case["n"], case["depth"], case["b"], fused)
    print(f"[{label}] routes: " + ", ".join(f"{k} {v}" for k, v in routes.items() if k != "tiles"))
    TM.assert_bars(label, result)


@pytest.mark.parametrize("tag", MATRIX)
def test_both_legs_on_every_network_vs_float64(tag):
    """One iteration of hn_train_grad (every tape tensor, activation gradient, input gradient, weight gradient; conv_state's exactly zero) and of
    hn_step_vjp with cotangents on wf, res and the states (input gradients, g_k_sq, g_src, every weight gradient, conv_state's included)."""
    _row(tag)


@pytest.mark.parametrize("tag,fused", ROUTE_ROWS)
def test_every_fused_option_value_vs_float64(tag, fused):
    """The non-default routes against float64 themselves: a defect shared by the default and its fallback would pass a comparison of the two."""
    _row(tag, fused)


@pytest.mark.parametrize("tag", list(ROUTE_VALUES))
def test_option_values_change_the_route_and_the_bits(tag):
    """Each HN_OPT_TRAIN_FUSED value changes the kernel family of at least one layer (train_routes), and the results say it ran: every value
    differs in bits from a neighbouring value or is separated from one only by values the header calls bit-identical (2 and 4: torch.equal is
    asserted; 16: "at the training sizes", nothing asserted).  Measured on an MI355X: at 80^2 and 64^2 the values 0 .. 23 give ONE set of bits, tape
    included -- below 128 columns the fused forward kernel happens to add up in the direct kernels' order.  Nobody promises that, so nothing is asserted
    about it, and on those two networks the step 0 -> 1 is excused from the rule: bits cannot show there that value 0 ran, train_routes (pinned to the
    source's text in test_train_matrix_host.py) is the only witness.  d4_160_A is the same network family with a level of at least 128 columns, where
    the rule holds for every value without the excuse; 23 -> 55 differs everywhere, and at 528^2 every step of 0 -> 7 -> 55 does."""
    case = TM.train_case(tag)
    s, eng = _engine(tag)
    cot = TM.cotangents(1, case["b"], case["n"], case["L"], case["n"])
    values, grads, tapes = ROUTE_VALUES[tag], {}, {}
    try:
        for v in values:
            eng.set_option("train_fused", v)
            got, mids, raw, blob = TM.hip_leg_a(eng, case)
            b = TM.hip_leg_b(eng, case, blob, raw, cot)
            grads[v] = [raw["grad"].cpu(), *got["a"]["in"].values(), *b["in"].values(), *b["w"].values()]
            tapes[v] = list(got["fwd"].values()) + list(got["a"]["tape"].values())
    finally:
        eng.set_option("train_fused", 55)
    eng.check_async_errors()
    differs = {}
    for u, v in zip(values, values[1:]):
        ru, rv = (TM.train_routes(case["n"], case["depth"], case["b"], x) for x in (u, v))
        changed = [k for k in ru if k != "tiles" and ru[k] != rv[k]]
        assert changed, (u, v)
        same = all(torch.equal(a, c) for a, c in zip(grads[u] + tapes[u], grads[v] + tapes[v]))
        differs[(u, v)] = not same
        print(f"[{tag}] {u} -> {v}: {len(changed)} layers change family ({changed[0]} {ru[changed[0]]} -> {rv[changed[0]]}); bits differ: {not same}")
        if _promised(u, v):
            assert all(torch.equal(a, c) for a, c in zip(grads[u], grads[v])), (u, v)
    excused = 1 if case["n"] < NARROW else 0
    for i, v in enumerate(values):
        near = [p for p in ((values[i - 1], v) if i else None, (v, values[i + 1]) if i + 1 < len(values) else None) if p]
        assert any(differs[p] or (p[0] ^ p[1]) & ~(BIT_IDENTICAL | MAY_BE_IDENTICAL | excused) == 0 for p in near), (v, differs)


def test_two_iterations_at_depth_5_smooth_activation():
    """Back-propagation through two iterations at depth 5 (tanh, 96^2 x 2) against float64 autograd through O.training_loss: the ping-pong of the
    three state-gradient buffers and the two gradient-buffer sets at a depth other than 3 or 4."""
    tag = "d5_96_tanh"
    case = TM.train_case(tag)
    s, eng = _engine(tag)
    d = lambda x: x.to(DEV).contiguous()  # noqa: E731
    blob = torch.from_numpy(pack_weights(dict(case["w"]), case["depth"], case["act"], case["sd"])).to(DEV)
    out = eng.train_grad(blob, d(case["wf"]), d(case["res"]), d(case["st"]), d(case["k_sq"]), d(case["src"]), 2, 1e4, input_grads=True)
    torch.cuda.synchronize()
    eng.check_async_errors()
    got = {"fwd": {"wf1": out["wavefields"][0].cpu(), "res1": out["residuals"][0].cpu(), "st1": out["states"][0].cpu()}, "loss": float(out["loss"][0]),
           "a": {"in": {"wf": out["grad_wf"].cpu(), "res": out["grad_res"].cpu(), "st": out["grad_states"].cpu()}, "w": TM._named_grads(case, out["grad"]), "tape": {}}}
    want = TM.oracle_legs(case, torch.float64, n_unroll=2)
    fwd, ea, _ = TM.compare(case, got, want, whole_tape=False)
    TM.report(fwd, TM.FWD_BAR)
    assert abs(got["loss"] - want["loss"]) <= 1e-5 * want["loss"]
    assert all(v is not None for v in want["a"]["w"].values())      # two iterations: conv_state has a gradient
    _, oa, _ = TM.compare(case, TM.oracle_legs(case, torch.float32, n_unroll=2), want, strict=False, whole_tape=False)
    oa = {k: v for k, v in oa.items() if k in ea}
    assert max(TM.bars(oa).values()) <= 1e-3, oa      # no tensor's bar above the suite's bar for unrolled iterations, whatever the CPU build
    TM.assert_bars(tag + " x 2 iterations", {"a": (ea, TM.bars(oa)), "b": ({}, {}), "fwd": fwd})
