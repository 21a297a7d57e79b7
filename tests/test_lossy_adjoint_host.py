"""The lossy adjoint operator and adjoint-state gradients, the part that needs no GPU: the three entry points declared, exported and bound; the
Engine methods and the ``absorption=None`` parameters; the chain rule of the medium against float64 autograd of the formulas written out; the
adjoint-state formulas against a central difference of the dense float64 solve; and the refusals the front end makes before any device work.
Every figure is printed before it is asserted (pytest -s)."""
import inspect
import os
import re
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

import lossy_adjoint_common as LA
from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(hdr, name):
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_the_binding_carries_the_three_entry_points():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    for name, sibling in (("hn_residual_vjp_lossy", "hn_residual_vjp"), ("hn_fgmres_adjoint_cycle_lossy", "hn_fgmres_adjoint_cycle")):
        params, old = _declared(hdr, name), _declared(hdr, sibling)
        at = old.index("const float* k_sq") + 1                 # the sibling's parameters with k_sq_im behind k_sq
        assert params == old[:at] + ["const float* k_sq_im"] + old[at:], (name, params)
        assert _lib.SYMBOLS[sibling][1] == _lib.SYMBOLS[name][1][:at] + _lib.SYMBOLS[name][1][at + 1:]
    grad, old = _declared(hdr, "hn_adjoint_grad_lossy"), _declared(hdr, "hn_adjoint_grad")
    at = old.index("float* g_k_sq") + 1
    assert grad == old[:at] + ["float* g_k_sq_im"] + old[at:], grad
    for name in ("hn_residual_vjp_lossy", "hn_fgmres_adjoint_cycle_lossy", "hn_adjoint_grad_lossy"):
        params = _declared(hdr, name)
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = c_void_p if "*" in p else c_float if p.startswith("float ") else c_int
            assert a is want, (name, p, a)
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # additions within ABI 7
    assert lib.hn_residual_vjp_lossy(None, None, None, None, None, 1, None) == -1
    assert lib.hn_fgmres_adjoint_cycle_lossy(None, None, None, None, None, 1, 1, 1, 0.0, 1, 1.0, None, None, None, None, None, None) == -1
    assert lib.hn_adjoint_grad_lossy(None, None, None, 1, 1, None, None, None, None) == -1
    # the header no longer calls the lossy operator a dead end, and still lists what is absent
    block = hdr[hdr.index("absorbing media: a complex k_sq"):hdr.index("int hn_residual_lossy(")]
    assert "hn_residual_vjp_lossy" in block and "hn_adjoint_grad_lossy" in block and "gradients of any kind" not in block
    assert "hn_step_vjp" in block and "float64" in block and "training" in block


def test_front_end_has_the_methods_and_the_absorption_parameters():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.absorption import complex_k_sq_grads
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres_adjoint
    assert callable(Engine.residual_vjp_lossy) and callable(Engine.fgmres_adjoint_cycle_lossy) and callable(Engine.adjoint_grad_lossy)
    assert callable(complex_k_sq_grads)
    for f in (gmres_adjoint, IterativeSolver.solve_implicit):
        assert inspect.signature(f).parameters["absorption"].default is None, f
    p = inspect.signature(Engine.fgmres_adjoint_cycle_lossy).parameters
    assert list(p)[1:5] == ["x", "k_sq", "k_sq_im", "rhs"]
    # adjoint_solve passes its keyword arguments through
    assert any(q.kind is inspect.Parameter.VAR_KEYWORD for q in inspect.signature(IterativeSolver.adjoint_solve).parameters.values())


def test_chain_rule_helper_matches_float64_autograd_of_the_formulas():
    """complex_k_sq_grads in float64 against autograd through k = omega / c, k_sq = k^2 - alpha^2, k_sq_im = 2 k alpha; bar 1e-13 of the largest
    entry (a dozen float64 operations on numbers of size 1).  A broadcast alpha gets the sum over its broadcast dimensions, formed by the caller."""
    from helmnet_amd.absorption import complex_k_sq_grads
    g = torch.Generator().manual_seed(5)
    shape = (3, 1, 16, 48)
    sos = 1.0 + torch.rand(shape, generator=g, dtype=torch.float64)
    g_k, g_ki = torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
    for omega in (1.0, 0.75):
        for alpha in (0.2 * torch.rand(shape, generator=g, dtype=torch.float64), torch.tensor([0.0, 0.1, 0.2], dtype=torch.float64).reshape(3, 1, 1, 1),
                      torch.tensor(0.05, dtype=torch.float64)):
            got_s, got_a = complex_k_sq_grads(g_k, g_ki, sos, alpha, omega)
            want_s, want_a = LA.chain_rule_ref(g_k, g_ki, sos, alpha, omega)
            assert got_s.dtype == got_a.dtype == torch.float64 and tuple(got_s.shape) == tuple(got_a.shape) == shape
            got_a = got_a.sum_to_size(alpha.shape) if alpha.dim() else got_a.sum()
            e_s = float((got_s - want_s).abs().max() / want_s.abs().max())
            e_a = float((got_a - want_a).abs().max() / want_a.abs().max())
            print(f"omega={omega} alpha{tuple(alpha.shape)}: relative error d/dsos {e_s:.3e}  d/dalpha {e_a:.3e}, bar 1e-13")
            assert e_s <= 1e-13 and e_a <= 1e-13
    # a number for alpha is accepted too
    got = complex_k_sq_grads(g_k, g_ki, sos, 0.05, 1.0)
    assert torch.equal(got[0], complex_k_sq_grads(g_k, g_ki, sos, torch.tensor(0.05, dtype=torch.float64), 1.0)[0])


def test_adjoint_state_formulas_against_central_differences_of_the_dense_float64_solve():
    """n = 32, a0 = 0.1, the ring medium in float64.  lam = solve(M^H, dJ/du); dJ/dk_sq and dJ/dk_sq_im by the formulas of the issue, chained by the
    helper; <grad, delta> against (J(+h delta) - J(-h delta)) / 2h with h = 1e-6, to 1e-6 relative, for the sound speed and for alpha."""
    from helmnet_amd.absorption import complex_k_sq_grads
    n, a0, h = 32, 0.1, 1e-6
    src = LA.np_complex(O.point_source_map(n, [12, 16], 10.0)[0])
    ref = LA.gradient_reference(n, a0, src)
    p = LA.ring_problem(n, a0)
    rx, b = ref["rx"], 0
    sos, alpha = p["sos"][b, 0].double().numpy(), p["alpha"][b, 0].double().numpy()
    to_t = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None, None]  # noqa: E731
    g_sos, g_alpha = complex_k_sq_grads(to_t(ref["g_k_sq"][b]), to_t(ref["g_k_sq_im"][b]), to_t(sos), to_t(alpha), LA.OMEGA)
    assert float((g_sos[0, 0] - torch.from_numpy(ref["g_sos"][b])).abs().max()) <= 1e-13 * float(np.abs(ref["g_sos"][b]).max())
    assert float((g_alpha[0, 0] - torch.from_numpy(ref["g_alpha"][b])).abs().max()) <= 1e-13 * float(np.abs(ref["g_alpha"][b]).max())
    rng = np.random.default_rng(17)
    for name, grad, moved in (("sos", g_sos, 0), ("alpha", g_alpha, 1)):
        delta = rng.standard_normal((n, n))
        plus = (sos + h * delta, alpha) if moved == 0 else (sos, alpha + h * delta)
        minus = (sos - h * delta, alpha) if moved == 0 else (sos, alpha - h * delta)
        fd = (LA.loss64(ref["M"][b], sos, alpha, *plus, src, rx, ref["d"][b]) - LA.loss64(ref["M"][b], sos, alpha, *minus, src, rx, ref["d"][b])) / (2 * h)
        an = float((grad[0, 0].numpy() * delta).sum())
        print(f"d/d{name}: adjoint {an:.10e}  central difference {fd:.10e}  relative {abs(an - fd) / abs(fd):.3e}, bar 1e-6")
        assert abs(an - fd) <= 1e-6 * abs(fd)


def test_refusals_before_any_device_work():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.gmres import gmres_adjoint
    sos, g = torch.ones(1, 1, 16, 16), torch.zeros(1, 2, 16, 16)
    with pytest.raises(ValueError, match="absorption needs backend='hip'"):
        gmres_adjoint(None, sos, g, backend="torch", absorption=0.1)
    s = IterativeSolver.from_exported_weights()      # on the CPU: nothing below may reach the library
    s.freeze()
    s.set_domain_size(32, source_location=[14, 16])
    one = torch.ones(1, 1, 32, 32)
    with pytest.raises(ValueError, match="absorption needs backend='hip'"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 32), one, backend="torch", absorption=0.1)
    with pytest.raises(RuntimeError, match="grad"):
        s.adjoint_solve(torch.zeros(1, 2, 32, 32), one, absorption=torch.full((1, 1, 32, 32), 0.1, requires_grad=True))
    with pytest.raises(ValueError, match="sos must be"):
        s.solve_implicit(torch.ones(1, 1, 16, 16), absorption=0.1)
    with pytest.raises(ValueError, match="x0 must be"):
        s.solve_implicit(torch.ones(2, 1, 32, 32), x0=torch.zeros(1, 2, 32, 32), absorption=0.1)
    with pytest.raises(ValueError, match="unknown precondition"):
        s.solve_implicit(one, precondition="ilu", absorption=0.1)
    with pytest.raises(ValueError, match="does not broadcast"):
        s.solve_implicit(one, absorption=torch.zeros(2, 1, 32, 32))
    # what stays refused: the loop, the cycles and the residual with absorption have no gradients
    a = torch.full((1, 1, 32, 32), 0.02)
    for call in (lambda: s.forward(one.clone().requires_grad_(True), num_iterations=1, absorption=0.02),
                 lambda: s.forward(one, num_iterations=1, absorption=a.clone().requires_grad_(True)),
                 lambda: s.solve_to_tolerance(one.clone().requires_grad_(True), 1e-3, max_iterations=2, absorption=0.02),
                 lambda: s.gmres(one.clone().requires_grad_(True), absorption=0.02),
                 lambda: s.n_steps(torch.zeros(1, 2, 32, 32, requires_grad=True), one, torch.zeros(1, 2, 32, 32), 1, absorption=0.02),
                 lambda: s.get_residual(torch.zeros(1, 2, 32, 32, requires_grad=True), one, k_sq_im=a)):
        with pytest.raises(RuntimeError, match="grad"):
            call()
    with pytest.raises(RuntimeError, match="with absorption runs without gradients"):
        s.forward(one.clone().requires_grad_(True), num_iterations=1, absorption=0.02)
    s.set_domain_size((32, 48), source_location=[14, 16])
    for call in (lambda: s.solve_implicit(torch.ones(1, 1, 32, 48), absorption=0.1),
                 lambda: s.adjoint_solve(torch.zeros(1, 2, 32, 48), torch.ones(1, 1, 32, 48), absorption=0.1)):
        with pytest.raises(NotImplementedError, match=r"rectangular domain \(32 x 48\)"):
            call()
