"""Absorbing media, the part that needs no GPU: the helper ``complex_k_sq`` against float64, the SIGN of the imaginary plane on the float64 direct
solve (absorption must damp, the other sign amplify), the three lossy entry points declared, exported and bound, and the refusals the front end
makes before any GPU work."""
import inspect
import os
import re
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

import lossy_common as LC
from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_complex_k_sq_against_float64_and_alpha_zero_is_get_initials():
    from helmnet_amd.absorption import complex_k_sq
    g = torch.Generator().manual_seed(11)
    sos = 1.0 + torch.rand(3, 1, 16, 48, generator=g, dtype=torch.float32)
    alpha = 0.2 * torch.rand(3, 1, 16, 48, generator=g, dtype=torch.float32)
    for omega in (1.0, 0.75):
        k, ki = complex_k_sq(sos, alpha, omega)
        assert k.dtype == ki.dtype == torch.float32 and k.shape == ki.shape == sos.shape
        kt = omega / sos.double() + 1j * alpha.double()
        want = kt * kt
        # three fp32 roundings of numbers of size <= 1 on the real plane (quotient, square, difference; alpha^2 is below 0.04), three on the other
        assert float((k.double() - want.real).abs().max()) <= 4 * 2.0 ** -24
        assert float((ki.double() - want.imag).abs().max()) <= 4 * 2.0 ** -24
        assert bool((ki >= 0).all())
        # alpha = 0: the bits of get_initials, and zeros -- as a number, as a tensor, and in float64 too
        for a in (0.0, torch.zeros(1, 1, 1, 48)):
            k0, ki0 = complex_k_sq(sos, a, omega)
            assert torch.equal(k0, O.get_initials(sos, omega)[0]) and not bool(ki0.any()) and ki0.shape == sos.shape
        k64, ki64 = complex_k_sq(sos.double(), alpha.double(), omega)
        assert k64.dtype == ki64.dtype == torch.float64
        assert float((k64 - want.real).abs().max()) <= 1e-15 and float((ki64 - want.imag).abs().max()) <= 1e-15
    # broadcasting: a number, one value per sample, one row
    per = torch.tensor([0.0, 0.1, 0.2]).reshape(3, 1, 1, 1)
    assert torch.equal(complex_k_sq(sos, per)[1], (2.0 * (1.0 / sos) * per).contiguous())
    assert torch.equal(complex_k_sq(sos, 0.1)[1], complex_k_sq(sos, torch.full_like(sos, 0.1))[1])
    with pytest.raises(ValueError, match="broadcast"):
        complex_k_sq(sos, torch.zeros(2, 1, 16, 48))
    doc = complex_k_sq.__doc__ + inspect.getmodule(complex_k_sq).__doc__
    assert "gamma = 1 + i sigma / k" in doc and "e^{+ikx}" in doc and "Im(k~) > 0" in doc      # the sign convention and why


def test_the_sign_absorption_damps_and_the_other_sign_amplifies():
    """The n = 32 float64 direct solve of the issue: ring phantom, point source of amplitude 10, PML 8, sigma_max 2, k 1; alpha = a0 inside the ring
    and a0 / 4 elsewhere, k_re and k_im from the helper, rounded to fp32.  Recorded on the CPU: rms 0.5821, 0.5290, 0.3860 for a0 = 0, 0.02, 0.1 and
    7.18 for a0 = -0.1."""
    from helmnet_amd.absorption import complex_k_sq
    n = 32
    src = O.point_source_map(n, [12, 16], 10.0).numpy()[0]
    rms = {}
    for a0 in LC.A0 + (-0.1,):
        sos, alpha = LC.ring_medium(n, a0)
        k_re, k_im = complex_k_sq(sos[:1], alpha[:1], 1.0)
        assert k_re.dtype == torch.float32
        u, mat = LC.direct_solve(k_re[0, 0].numpy(), k_im[0, 0].numpy(), src)
        rms[a0] = float(np.sqrt((u ** 2).sum(0).mean()))      # of the complex field
        print(f"n={n} a0={a0}: rms of u {rms[a0]:.4f}")
    assert rms[0.0] > rms[0.02] > rms[0.1] > 0
    assert rms[-0.1] > rms[0.0]


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
    for name, sibling in (("hn_residual_lossy", "hn_residual"), ("hn_step_lossy", "hn_step"), ("hn_fgmres_cycle_lossy", "hn_fgmres_cycle")):
        params, old = _declared(hdr, name), _declared(hdr, sibling)
        # the sibling's parameters with k_sq_im behind k_sq
        at = old.index("const float* k_sq") + 1
        assert params == old[:at] + ["const float* k_sq_im"] + old[at:], (name, params)
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = c_void_p if "*" in p else c_float if p.startswith("float ") else c_int
            assert a is want, (name, p, a)
        assert _lib.SYMBOLS[sibling][1] == args[:at] + args[at + 1:]
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # additions within ABI 7
    assert lib.hn_residual_lossy(None, None, None, None, None, 1, None, 1, None) == -1
    assert lib.hn_step_lossy(None, None, None, None, None, None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert lib.hn_fgmres_cycle_lossy(None, None, None, None, None, 1, 1, 1, 0.0, 1, 1.0, None, None, None, None, None, None) == -1


def test_front_end_signatures_and_refusals_before_any_gpu_work():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres
    assert callable(Engine.residual_lossy) and callable(Engine.step_lossy) and callable(Engine.fgmres_cycle_lossy)
    for f in (IterativeSolver.forward, IterativeSolver.n_steps, IterativeSolver.solve_to_tolerance, IterativeSolver.gmres, gmres):
        assert inspect.signature(f).parameters["absorption"].default is None, f
    assert inspect.signature(IterativeSolver.get_residual).parameters["k_sq_im"].default is None
    sos = torch.ones(1, 1, 16, 16)
    with pytest.raises(ValueError, match="absorption needs backend='hip'"):
        gmres(None, sos, backend="torch", absorption=0.1)
    with pytest.raises(NotImplementedError, match="float64 lossy"):
        gmres(None, sos, backend="hip", refine=True, absorption=0.1)
    # a solver that is still on the CPU: the gradient refusal comes before the engine is asked for (which would raise its own RuntimeError)
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.set_domain_size(16, source_location=[4, 8])
    a = torch.full((1, 1, 16, 16), 0.02)
    for call in (lambda: s.forward(sos.clone().requires_grad_(True), num_iterations=1, absorption=0.02),
                 lambda: s.forward(sos, num_iterations=1, absorption=a.clone().requires_grad_(True)),
                 lambda: s.solve_to_tolerance(sos.clone().requires_grad_(True), 1e-3, max_iterations=2, absorption=0.02),
                 lambda: s.gmres(sos.clone().requires_grad_(True), absorption=0.02),
                 lambda: s.n_steps(torch.zeros(1, 2, 16, 16, requires_grad=True), sos, torch.zeros(1, 2, 16, 16), 1, absorption=0.02),
                 lambda: s.get_residual(torch.zeros(1, 2, 16, 16, requires_grad=True), sos, k_sq_im=a)):
        with pytest.raises(RuntimeError, match="grad"):
            call()
    with pytest.raises(RuntimeError, match="with absorption runs without gradients"):
        s.forward(sos.clone().requires_grad_(True), num_iterations=1, absorption=0.02)
    with pytest.raises(NotImplementedError, match="verify=True"):
        s.solve_to_tolerance(sos, 1e-3, max_iterations=2, verify=True, absorption=0.02)
