"""The adjoint of the variable-density operator and its adjoint-state gradients, the part that needs no GPU: the three entry points declared,
exported and bound; the front end's ``density`` parameters; ``log_density_gradient_vjp`` against float64 autograd; the gradient formulas against
central differences of the dense float64 solve; and the similarity weight W / rho of the learned preconditioner on the dense operator.
Every figure is printed before it is asserted (pytest -s)."""
import inspect
import os
import re
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

import density_adjoint_common as DA
import density_common as DC
import lossy_adjoint_common as LA
from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(hdr, name):
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_header_declares_and_the_binding_carries_the_three_entry_points():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    want = {
        "hn_residual_vjp_medium": ["hn_ctx*", "const float* g", "const float* k_sq", "const float* k_sq_im", "const float* rho_grad", "float* out", "int batch",
                                   "void* stream"],
        "hn_fgmres_adjoint_cycle_medium": ["hn_ctx*", "float* x", "const float* k_sq", "const float* k_sq_im", "const float* rho_grad", "const float* rho",
                                           "const float* rhs", "int rhs_batch", "int batch", "int restart", "float tol", "int precond_iters",
                                           "float precond_scale", "float* basis", "float* zbasis", "float* hess", "float* rmse", "int* k_used", "void* stream"],
        "hn_adjoint_grad_medium": ["hn_ctx*", "const float* lambda", "const float* u", "int src_batch", "int batch", "float* g_k_sq", "float* g_k_sq_im",
                                   "float* g_rho_grad", "float* g_src", "void* stream"]}
    for name, params in want.items():
        got = _declared(hdr, name)
        assert [p.replace("hn_ctx* ctx", "hn_ctx*") for p in got] == params, (name, got)
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            assert a is (c_void_p if "*" in p else c_float if p.startswith("float ") else c_int), (name, p, a)
    # the lossy siblings with rho_grad behind k_sq_im (the cycle: rho behind that), g_rho_grad behind g_k_sq_im
    for name, sibling, behind, extra in (("hn_residual_vjp_medium", "hn_residual_vjp_lossy", "const float* k_sq_im", 1),
                                         ("hn_fgmres_adjoint_cycle_medium", "hn_fgmres_adjoint_cycle_lossy", "const float* k_sq_im", 2),
                                         ("hn_adjoint_grad_medium", "hn_adjoint_grad_lossy", "float* g_k_sq_im", 1)):
        at = _declared(hdr, sibling).index(behind) + 1
        assert _lib.SYMBOLS[sibling][1] == _lib.SYMBOLS[name][1][:at] + _lib.SYMBOLS[name][1][at + extra:], name
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # additions within ABI 7
    assert lib.hn_residual_vjp_medium(None, None, None, None, None, None, 1, None) == -1
    assert lib.hn_fgmres_adjoint_cycle_medium(None, None, None, None, None, None, None, 1, 1, 1, 0.0, 1, 1.0, None, None, None, None, None, None) == -1
    assert lib.hn_adjoint_grad_medium(None, None, None, 1, 1, None, None, None, None, None) == -1
    # the header no longer calls the density operator a dead end, and still lists what is absent
    block = hdr[hdr.index("heterogeneous density (added within ABI v7"):hdr.index("int hn_residual_medium(")]
    assert "the adjoint of A_rho and adjoint-state gradients" not in block
    assert "hn_residual_vjp_medium" in block and "hn_adjoint_grad_medium" in block
    assert "float64" in block and "hn_stream_swap" in block and "gradients through the loop" in block and "training" in block
    src = open(os.path.join(REPO, "helmnet_amd", "csrc", "hn_internal.h")).read()
    assert re.search(r"KID_COUNT = 37\b", src)                # no new profile kernel ids


def test_front_end_has_the_methods_and_the_density_parameters():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.density import log_density_gradient_vjp
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres_adjoint
    assert callable(Engine.residual_vjp_medium) and callable(Engine.fgmres_adjoint_cycle_medium) and callable(Engine.adjoint_grad_medium)
    assert callable(log_density_gradient_vjp)
    for f in (gmres_adjoint, IterativeSolver.solve_implicit):
        p = inspect.signature(f).parameters
        assert p["density"].default is None and list(p)[-1] == "density", f       # behind the existing parameters
    assert list(inspect.signature(Engine.residual_vjp_medium).parameters)[1:5] == ["g", "k_sq", "k_sq_im", "rho_grad"]
    assert list(inspect.signature(Engine.fgmres_adjoint_cycle_medium).parameters)[1:7] == ["x", "k_sq", "k_sq_im", "rho_grad", "rho", "rhs"]
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in inspect.signature(IterativeSolver.adjoint_solve).parameters.values())


def test_log_density_gradient_vjp_matches_float64_autograd():
    """48 x 80, float64: dJ/drho for J = <g, q(rho)> against autograd through the torch restatement of ``density_common.log_gradient`` (the 1 / rho
    chain included); bar 1e-12 of the largest entry (two float64 FFT pairs on numbers of size 1).  A rho broadcast along the batch gets the sum over
    it, formed by the caller; a non-positive rho raises ValueError; the result has the dtype of rho."""
    from helmnet_amd.density import log_density_gradient, log_density_gradient_vjp
    gen = torch.Generator().manual_seed(21)
    b, h, w = 3, 48, 80
    rho = 1.0 + torch.rand(b, 1, h, w, generator=gen, dtype=torch.float64)
    g = torch.randn(b, 2, h, w, generator=gen, dtype=torch.float64)
    # the restatement is the map the product's forward function computes
    assert float((DA.log_gradient_torch(rho) - log_density_gradient(rho)).abs().max()) <= 1e-13
    got, want = log_density_gradient_vjp(g, rho), DA.rho_chain_ref(g, rho)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{h}x{w}: log_density_gradient_vjp against float64 autograd, relative to the largest entry {err:.3e}, bar 1e-12")
    assert got.dtype == torch.float64 and tuple(got.shape) == (b, 1, h, w) and err <= 1e-12
    one = rho[:1]
    got1, want1 = log_density_gradient_vjp(g, one).sum(0, keepdim=True), DA.rho_chain_ref(g, one)
    err1 = float((got1 - want1).abs().max() / want1.abs().max())
    print(f"{h}x{w}: one rho for the batch, summed over it: {err1:.3e}, bar 1e-12")
    assert tuple(got1.shape) == tuple(want1.shape) == (1, 1, h, w) and err1 <= 1e-12
    assert log_density_gradient_vjp(g.float(), rho.float()).dtype == torch.float32
    bad = rho.clone()
    bad[1, 0, 3, 4] = 0.0
    with pytest.raises(ValueError, match="positive"):
        log_density_gradient_vjp(g, bad)
    with pytest.raises(ValueError, match="g_rho_grad"):
        log_density_gradient_vjp(g[:, :1], rho)


def test_density_gradient_formulas_against_central_differences_of_the_dense_float64_solve():
    """n = 32, a0 = 0.1, the three-map ring medium in float64 (q without the fp32 rounding).  lam = solve(M^H, dJ/du); dJ/dq by the formula of the
    issue, dJ/drho through ``log_density_gradient_vjp``; <grad, delta> against (J(+h delta) - J(-h delta)) / 2h with h = 1e-6, to 1e-6 relative, for q
    and for rho (rho perturbed, q recomputed in float64)."""
    from helmnet_amd.density import log_density_gradient_vjp
    n, a0, h = 32, 0.1, 1e-6
    src = LA.np_complex(O.point_source_map(n, [12, 16], 10.0)[0])
    ref = DA.gradient_reference(n, a0, src, exact_q=True)
    p = DA.ring_problem(n, a0)
    rx, b = ref["rx"], 0
    M, q0, d = ref["M"][b], ref["q"][b], ref["d"][b]
    rho = p["rho"][b:b + 1].double()
    g_rho = log_density_gradient_vjp(torch.from_numpy(ref["g_q"][b])[None], rho)[0, 0].numpy()
    e = float(np.abs(g_rho - ref["g_rho"][b]).max() / np.abs(ref["g_rho"][b]).max())
    print(f"dJ/drho: log_density_gradient_vjp against autograd through the restated gradient {e:.3e}, bar 1e-12")
    assert e <= 1e-12
    rng = np.random.default_rng(23)
    dq = rng.standard_normal((2, n, n))
    fd = (DA.loss64(M, q0, q0 + h * dq, src, rx, d) - DA.loss64(M, q0, q0 - h * dq, src, rx, d)) / (2 * h)
    an = float((ref["g_q"][b] * dq).sum())
    print(f"d/dq: adjoint {an:.10e}  central difference {fd:.10e}  relative {abs(an - fd) / abs(fd):.3e}, bar 1e-6")
    assert abs(an - fd) <= 1e-6 * abs(fd)
    delta = rng.standard_normal((n, n))
    qp = DA.log_gradient_torch(rho + h * torch.from_numpy(delta))[0].numpy()
    qm = DA.log_gradient_torch(rho - h * torch.from_numpy(delta))[0].numpy()
    fd = (DA.loss64(M, q0, qp, src, rx, d) - DA.loss64(M, q0, qm, src, rx, d)) / (2 * h)
    an = float((g_rho * delta).sum())
    print(f"d/drho: adjoint {an:.10e}  central difference {fd:.10e}  relative {abs(an - fd) / abs(fd):.3e}, bar 1e-6")
    assert abs(an - fd) <= 1e-6 * abs(fd)


def test_similarity_weight_of_the_density_operator_is_w_over_rho():
    """The table of the issue from ``density_common.medium_matrix`` at n = 32: with X = W / rho the exact inverse between the weights is a contraction
    on A_rho^H (||A^H M - I||_2 < 1) and a better one than with W alone; W * rho, the wrong way round, is worse than either."""
    t = DA.similarity_table(32)
    print(f"n=32 max|q| {t['max|q|']:.2f}: " + "; ".join(f"{k}: defect {t[k][0]:.3f} 2-norm {t[k][1]:.2f}" for k in ("W", "W/rho", "W*rho")))
    assert t["W/rho"][1] < 1.0 and t["W/rho"][1] < t["W"][1]
    assert t["W/rho"][0] < t["W"][0] < t["W*rho"][0] and t["W"][1] < t["W*rho"][1]


def test_refusals_before_any_device_work():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.gmres import gmres_adjoint
    sos, g = torch.ones(1, 1, 16, 16), torch.zeros(1, 2, 16, 16)
    with pytest.raises(ValueError, match="density needs backend='hip'"):
        gmres_adjoint(None, sos, g, backend="torch", density=sos)
    s = IterativeSolver.from_exported_weights()      # on the CPU: nothing below may reach the library
    s.freeze()
    s.set_domain_size(32, source_location=[14, 16])
    one = torch.ones(1, 1, 32, 32)
    with pytest.raises(RuntimeError, match="grad"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 32), one, density=one.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="sos must be"):
        s.solve_implicit(torch.ones(1, 1, 16, 16), density=one)
    with pytest.raises(ValueError, match="does not broadcast"):
        s.solve_implicit(one, density=torch.ones(2, 1, 32, 32))
    with pytest.raises(TypeError, match="density must be a tensor"):
        s.solve_implicit(one, density=2.0)
    # what stays refused: the loop, the cycles and the residual with density have no gradients
    for call in (lambda: s.forward(one.clone().requires_grad_(True), num_iterations=1, density=one),
                 lambda: s.forward(one, num_iterations=1, density=one.clone().requires_grad_(True)),
                 lambda: s.solve_to_tolerance(one.clone().requires_grad_(True), 1e-3, max_iterations=2, density=one),
                 lambda: s.gmres(one.clone().requires_grad_(True), density=one),
                 lambda: s.n_steps(torch.zeros(1, 2, 32, 32, requires_grad=True), one, torch.zeros(1, 2, 32, 32), 1, density=one),
                 lambda: s.get_residual(torch.zeros(1, 2, 32, 32, requires_grad=True), one, rho_grad=torch.zeros(1, 2, 32, 32))):
        with pytest.raises(RuntimeError, match="grad"):
            call()
    s.set_domain_size((32, 48), source_location=[14, 16])
    for call in (lambda: s.solve_implicit(torch.ones(1, 1, 32, 48), density=torch.ones(1, 1, 32, 48)),
                 lambda: s.adjoint_solve(torch.zeros(1, 2, 32, 48), torch.ones(1, 1, 32, 48), density=torch.ones(1, 1, 32, 48))):
        with pytest.raises(NotImplementedError, match=r"rectangular domain \(32 x 48\)"):
            call()
