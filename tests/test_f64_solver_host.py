"""CPU-only checks of the float64 solver loop's interface: the two C entry points and the three IterativeSolver methods (no compute calls)."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of parameters the issue and INTEGRATION.md section 9 document
ENTRY_POINTS = {"hn_unet_f64": 7, "hn_step_f64": 14}


def _header():
    with open(os.path.join(REPO, "include", "helmnet_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_header_declares_the_entry_point(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m is not None, name
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == ENTRY_POINTS[name], params
    assert params[0] == "hn_ctx* ctx" and params[-1] == "void* stream"
    assert all("double*" in p for p in params if "*" in p and p not in (params[0], params[-1]))      # every tensor is double
    assert "#define HN_ABI_VERSION 7" in _header()


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_library_exports_the_entry_point(name):
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    fn = getattr(lib, name)
    assert fn is not None and len(_lib.SYMBOLS[name][1]) == ENTRY_POINTS[name] and len(fn.argtypes) == ENTRY_POINTS[name]
    # a NULL context is refused without touching a device
    args = [None] * 5 + [1, None] if name == "hn_unet_f64" else [None] * 6 + [1, 1, 1] + [None] * 5
    assert fn(*args) == -1


def _cpu_solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    return s


def test_cpu_solver_raises_what_forward_raises():
    s = _cpu_solver()
    sos = torch.ones(1, 1, 96, 96)
    with pytest.raises(RuntimeError) as want:
        s.forward(sos, num_iterations=1)
    z2, z1, st = torch.zeros(1, 2, 96, 96, dtype=torch.float64), torch.ones(1, 1, 96, 96, dtype=torch.float64), torch.zeros(1, 2, s.f.total_state_length, dtype=torch.float64)
    for call in (lambda: s.forward64(sos, num_iterations=1), lambda: s.n_steps64(z2, z1, z2, st, 1), lambda: s.deviation_from_float64(sos, 2, [1, 2])):
        with pytest.raises(RuntimeError) as got:
            call()
        assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    assert "on the CPU" in str(want.value)


def test_inputs_that_require_grad_are_refused():
    s = _cpu_solver()
    sos = torch.ones(1, 1, 96, 96, requires_grad=True)
    z2, z1, st = torch.zeros(1, 2, 96, 96, dtype=torch.float64), torch.ones(1, 1, 96, 96, dtype=torch.float64), torch.zeros(1, 2, s.f.total_state_length, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="without gradients"):
        s.forward64(sos, num_iterations=1)
    with pytest.raises(RuntimeError, match="without gradients"):
        s.forward64(sos.detach(), num_iterations=1, source=torch.zeros(1, 2, 96, 96, dtype=torch.float64, requires_grad=True))
    with pytest.raises(RuntimeError, match="without gradients"):
        s.n_steps64(z2, z1, z2, st.clone().requires_grad_(True), 1)
    with pytest.raises(RuntimeError, match="without gradients"):
        s.deviation_from_float64(sos, 2, [1])
