"""Absorbing media in float64 (hn_residual_f64_lossy, hn_fgmres_refine_cycle_lossy and the keywords that reach them), what needs no GPU: the two
declarations and their bindings, the Python keywords and the refusals that come before any device work, and the agreement of the reference
tests/test_f64_lossy_gpu.py measures against (``LC.forward_case``) with an independent float64 assembly,
    M_H U + U M_W^T + (k_sq + i k_sq_im) U - S,   M_n = ``O.axis_operator_matrix(n, ...)``,
to 1e-12 of max (tests/test_rect_host.py's bar), on the rectangles the GPU test uses."""
import inspect
import os
import re
from ctypes import c_double, c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

import lossy_common as LC
import rect_common as R
from oracle import helmnet_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(hdr, name):
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_and_the_binding_carries_the_two_entry_points():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    for name, sibling, ctype in (("hn_residual_f64_lossy", "hn_residual_f64", "double"), ("hn_fgmres_refine_cycle_lossy", "hn_fgmres_refine_cycle", "float")):
        params, old = _declared(hdr, name), _declared(hdr, sibling)
        at = old.index(f"const {ctype}* k_sq") + 1
        assert params == old[:at] + [f"const {ctype}* k_sq_im"] + old[at:], (name, params)      # the sibling's parameters with k_sq_im behind k_sq
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params), (name, len(args), len(params))
        for p, a in zip(params, args):
            want = c_void_p if "*" in p else c_float if p.startswith("float ") else c_double if p.startswith("double ") else c_int
            assert a is want, (name, p, a)
        assert _lib.SYMBOLS[sibling][1] == args[:at] + args[at + 1:]
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # additions within ABI 7
    assert lib.hn_residual_f64_lossy(None, None, None, None, None, 1, None, None, 1, None) == -1
    assert lib.hn_fgmres_refine_cycle_lossy(None, None, None, None, None, 1, 1, 1, 0.0, 0.0, 0, 1.0, None, None, None, None, None, None, None) == -1


def test_front_end_keywords_and_refusals_before_any_gpu_work():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres_refine_lossy
    assert callable(Engine.residual64_lossy) and callable(Engine.fgmres_refine_cycle_lossy) and callable(gmres_refine_lossy)
    sig = inspect.signature
    assert list(sig(Engine.residual64_lossy).parameters)[1:] == ["wf", "k_sq", "k_sq_im", "src", "want_res", "want_rmse"]
    assert sig(IterativeSolver.get_residual64).parameters["k_sq_im"].default is None
    assert list(sig(IterativeSolver.verify).parameters)[1:] == ["wavefield", "sos_maps", "k_sq", "absorption", "k_sq_im"]
    for f in (IterativeSolver.verify, IterativeSolver.gmres64, IterativeSolver.reference_error):
        assert sig(f).parameters["absorption"].default is None, f
    assert sig(IterativeSolver.verify).parameters["k_sq_im"].default is None
    # a solver that is still on the CPU: every refusal below comes before the engine is asked for (which would raise its own RuntimeError)
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.set_domain_size(16, source_location=[4, 8])
    sos, wf = torch.ones(1, 1, 16, 16), torch.zeros(1, 2, 16, 16)
    a = torch.full((1, 1, 16, 16), 0.02)
    for call in (lambda: s.verify(wf, sos_maps=sos, k_sq_im=a),              # k_sq_im goes with k_sq
                 lambda: s.verify(wf, k_sq=sos, absorption=0.02),             # absorption goes with sos_maps
                 lambda: s.verify(wf, sos_maps=sos, k_sq=sos, absorption=0.02),
                 lambda: s.verify(wf, absorption=0.02),
                 lambda: s.verify(wf, k_sq_im=a),
                 lambda: s.verify(wf, k_sq=sos, absorption=0.02, k_sq_im=a),
                 lambda: s.verify(wf, sos_maps=sos, absorption=0.02, k_sq_im=a)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: s.gmres64(sos.clone().requires_grad_(True), absorption=0.02),
                 lambda: s.gmres64(sos, absorption=a.clone().requires_grad_(True)),
                 lambda: s.gmres64(sos, absorption=0.02, x0=wf.clone().requires_grad_(True)),
                 lambda: s.reference_error(wf.clone().requires_grad_(True), sos, absorption=0.02),
                 lambda: s.reference_error(wf, sos.clone().requires_grad_(True), absorption=0.02),
                 lambda: s.verify(wf.clone().requires_grad_(True), sos_maps=sos, absorption=0.02),
                 lambda: s.verify(wf, k_sq=sos.clone().requires_grad_(True), k_sq_im=a)):
        with pytest.raises(RuntimeError, match="with absorption runs without gradients"):
            call()
    s.differentiable(True)
    with pytest.raises(RuntimeError, match="with absorption runs without gradients"):
        s.gmres64(sos, absorption=0.02)
    with pytest.raises(ValueError, match="needs absorption"):
        gmres_refine_lossy(s, sos, None)


@pytest.mark.parametrize("h,w", [(32, 80), (48, 16), (16, 2048), (2032, 16)])
def test_the_reference_is_the_per_axis_matrices_plus_the_complex_term(h, w):
    c = LC.forward_case(h, w)
    mh, mw = O.axis_operator_matrix(h, *R.DOMAIN), O.axis_operator_matrix(w, *R.DOMAIN)
    worst = 0.0
    for i in range(c["u"].shape[0]):
        u = c["u"][i, 0].double().numpy() + 1j * c["u"][i, 1].double().numpy()
        kk = c["k_sq"][i, 0].double().numpy() + 1j * c["k_sq_im"][i, 0].double().numpy()
        s = c["srcb"][i, 0].double().numpy() + 1j * c["srcb"][i, 1].double().numpy()
        want = mh @ u + u @ mw.T + kk * u - s
        got = c["lresb"][i, 0].numpy() + 1j * c["lresb"][i, 1].numpy()
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"{h}x{w}: |LC.forward_case lresb - (M_H U + U M_W^T + k~^2 U - S)| / max = {worst:.2e}")
    assert worst <= 1e-12
