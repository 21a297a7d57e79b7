"""What the forward-mode tests share (tests/test_jvp_gpu.py, tests/test_jvp_host.py): seeded cases, the CPU oracle's forward AD (teacher-forced at a
given tape, in any dtype) and the error measures.

The oracle is ``oracle.helmnet_oracle.single_step`` under ``torch.autograd.forward_ad``: iteration t is differentiated at the tape's slot t - 1 (the
inputs for t = 0) and the tangents are chained -- what hn_step_jvp linearises at, so the drift of a free-running fp32 trajectory drops out."""
import numpy as np
import torch
import torch.autograd.forward_ad as fwAD

from config_weights import config_input, config_weights
from golden_inputs import teacher_inputs
from oracle import helmnet_oracle as O

KINKED = ("prelu", "relu", "leakyrelu")
SMOOTH = ("celu", "tanh", "gelu", "tanhshrink", "softplus")


def errs(got, want):
    """(L_inf relative to the tensor's max, relative L2)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return (float((got - want).abs().max() / want.abs().max().clamp_min(1e-30)), float((got - want).norm() / want.norm().clamp_min(1e-30)))


def make_case(n, b, seed, depth=4, act="prelu", src_batch=1, n_weights=64, sd=None):
    """Seeded weights (config_weights), inputs (teacher_inputs at depth 4, config_input otherwise), a source and one direction on every input."""
    w = config_weights(depth, seed, "A", act, sd, n=n_weights)
    x = teacher_inputs(n, b, seed) if depth == 4 else config_input(n, b, depth, seed)
    g = torch.Generator().manual_seed(seed + 17)
    L = x["states"].shape[-1]
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    src = O.point_source_map(n, [n // 8, n // 2], 10.0) if src_batch == 1 else rnd(b, 2, n, n)
    tan = {"wf": rnd(b, 2, n, n), "res": 5e-3 * rnd(b, 2, n, n), "st": 0.5 * rnd(b, 2, L), "k_sq": 0.1 * rnd(b, 1, n, n), "src": rnd(src_batch, 2, n, n)}
    t = {k: torch.from_numpy(v) for k, v in x.items()}
    return dict(n=n, b=b, depth=depth, act=act, sd=sd, L=L, w={k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, w_np=w, wf=t["wf"], res=t["res"],
                st=t["states"], k_sq=(1.0 / t["sos"]) ** 2, src=src.float(), tan=tan)


def oracle_jvp(case, tape, tan, K, dtype):
    """Forward AD of K chained single_steps in ``dtype``, teacher-forced at ``tape`` = (wf_hist, res_hist, st_hist) (CPU tensors; None: free-running from
    the inputs).  ``tan``: the five input directions (a missing key = zero).  Returns the tangent histories {"wf", "res", "st"}, each [K, ...]."""
    n, depth, act = case["n"], case["depth"], case["act"]
    tab = O.SpectralTables(n, 8, 2, 1.0, dtype=dtype)
    w = {k: v.to(dtype) for k, v in case["w"].items()}
    zero = lambda like: torch.zeros_like(like, dtype=dtype)  # noqa: E731
    get = lambda k, like: tan[k].to(dtype) if tan.get(k) is not None else zero(like)  # noqa: E731
    t_wf, t_res, t_st = get("wf", case["wf"]), get("res", case["res"]), get("st", case["st"])
    t_k, t_s = get("k_sq", case["k_sq"]), get("src", case["src"])
    prev = tuple(case[k].to(dtype) for k in ("wf", "res", "st"))
    out = {"wf": [], "res": [], "st": []}
    for i in range(K):
        if tape is not None and i > 0:
            prev = tuple(h[i - 1].to(dtype) for h in tape)
        with fwAD.dual_level():
            a, r, h = (fwAD.make_dual(p, t) for p, t in zip(prev, (t_wf, t_res, t_st)))
            k = fwAD.make_dual(case["k_sq"].to(dtype), t_k)
            s = fwAD.make_dual(case["src"].to(dtype), t_s)
            wf, res, st = O.single_step(a, k, r, O.unflatten_states(h, n, depth), w, s, tab, depth, act, state_depth=case.get("sd"))
            outs = [fwAD.unpack_dual(v) for v in (wf, res, O.flatten_states(st))]
            prims = tuple(v.primal.detach() for v in outs)
            t_wf, t_res, t_st = (v.tangent.detach().clone() if v.tangent is not None else zero(v.primal) for v in outs)
        if tape is None:
            prev = prims
        for key, v in zip(("wf", "res", "st"), (t_wf, t_res, t_st)):
            out[key].append(v)
    return {k: torch.stack(v) for k, v in out.items()}


def oracle_precondition(case, tape, tan, K):
    """The oracle's own fp32 forward AD against its float64 forward AD on these inputs: (float64 result, {tensor: (L_inf, L2)}).  For the piecewise-linear
    activations every figure must be <= 1e-5 (asserted here: an input whose trajectory crosses a kink between the two precisions cannot carry a comparison
    and has to be replaced by its author)."""
    want = oracle_jvp(case, tape, tan, K, torch.float64)
    own = oracle_jvp(case, tape, tan, K, torch.float32)
    e = {k: errs(own[k], want[k]) for k in want}
    if case["act"] in KINKED:
        assert all(v[0] <= 1e-5 and v[1] <= 1e-5 for v in e.values()), f"the oracle's fp32 forward AD is off its float64 one (a kink flipped?): {e}"
    return want, e
