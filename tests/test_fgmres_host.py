"""Flexible GMRES with the learned preconditioner, the part that needs no GPU: hn_fgmres_cycle and hn_fgmres_refine_cycle are declared, exported and
bound; the public entries refuse what they must before any GPU work; and the accounting of UNet evaluations is exercised through the host drivers
with scripted cycles."""
import os
import re
from ctypes import c_double, c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(hdr, name):
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_library_exports_both_flexible_entry_points():
    from helmnet_amd import _lib
    from helmnet_amd.build import build
    build()
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    for name, count in (("hn_fgmres_cycle", 16), ("hn_fgmres_refine_cycle", 18)):
        params = _declared(hdr, name)
        res, args = _lib.SYMBOLS[name]
        assert res is c_int and len(args) == len(params) == count, (name, len(args), len(params))
        for p, a in zip(params, args):
            want = c_void_p if "*" in p else c_double if p.startswith("double ") else c_float if p.startswith("float ") else c_int
            assert a is want, (name, p, a)
    cyc, ref = _declared(hdr, "hn_fgmres_cycle"), _declared(hdr, "hn_fgmres_refine_cycle")
    assert cyc[1] == "float* x" and cyc[7] == "float tol" and cyc[8:12] == ["int precond_iters", "float precond_scale", "float* basis", "float* zbasis"]
    assert ref[1] == "double* x" and ref[7] == "double tol" and ref[8] == "float inner_floor"
    assert ref[9:13] == ["int precond_iters", "float precond_scale", "float* basis", "float* zbasis"] and ref[16] == "double* rmse64"
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # new entry points within ABI 7
    assert lib.hn_fgmres_cycle(None, None, None, None, 1, 1, 1, 0.0, 1, 1.0, None, None, None, None, None, None) == -1
    assert lib.hn_fgmres_refine_cycle(None, None, None, None, 1, 1, 1, 0.0, 0.0, 1, 1.0, None, None, None, None, None, None, None) == -1
    # the old entry points are still what they were
    assert len(_lib.SYMBOLS["hn_gmres_cycle"][1]) == 13 and len(_lib.SYMBOLS["hn_gmres_refine_cycle"][1]) == 15
    assert len(_declared(hdr, "hn_gmres_cycle")) == 13 and len(_declared(hdr, "hn_gmres_refine_cycle")) == 15


def test_public_entries_exist_and_refuse_before_any_gpu_work():
    import inspect
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    from helmnet_amd.gmres import gmres
    assert callable(Engine.fgmres_cycle) and callable(Engine.fgmres_refine_cycle)
    for f in (gmres, IterativeSolver.gmres, IterativeSolver.gmres64, IterativeSolver.reference_error):
        p = inspect.signature(f).parameters
        assert p["precondition"].default is None and p["precond_iterations"].default == 10 and p["precond_scale"].default is None, f
    sos = torch.ones(1, 1, 16, 16)
    with pytest.raises(ValueError, match="precondition='learned' needs backend='hip'"):
        gmres(None, sos, backend="torch", precondition="learned")
    with pytest.raises(ValueError, match="unknown precondition"):
        gmres(None, sos, backend="hip", precondition="jacobi")
    with pytest.raises(ValueError, match="unknown precondition"):
        gmres(None, sos, backend="torch", precondition="ilu")
    with pytest.raises(ValueError, match="precond_iterations"):
        gmres(None, sos, backend="hip", precondition="learned", precond_iterations=-1)
    with pytest.raises(RuntimeError, match="grad"):
        gmres(None, sos.clone().requires_grad_(True), backend="hip", precondition="learned", precond_scale=1.0)
    with pytest.raises(ValueError, match="refine"):                     # the older refusal is still the first
        gmres(None, sos, backend="torch", refine=True, precondition="learned")


def test_default_scale_is_the_rms_two_norm_of_the_source_maps():
    from helmnet_amd.gmres import default_precond_scale
    one = torch.zeros(1, 2, 4, 4); one[0, 0, 1, 2] = 3.0; one[0, 1, 1, 2] = 4.0
    assert default_precond_scale(one) == 5.0
    many = torch.cat([one, 2.0 * one, 2.0 * one])                       # norms 5, 10, 10: sqrt((25 + 100 + 100) / 3)
    assert default_precond_scale(many) == pytest.approx(np.sqrt(75.0), rel=1e-15)
    tiny = torch.full((1, 2, 4, 4), 1e-30)                              # float64 on the host: the squares of fp32 values this small are not lost
    assert default_precond_scale(tiny) == pytest.approx(np.sqrt(32.0) * float(np.float32(1e-30)), rel=1e-12)


class _Script:
    def __init__(self, cycles):
        self.cycles, self.calls = list(cycles), 0

    def cycle(self):
        out = self.cycles[self.calls]
        self.calls += 1
        return out


def test_unet_evaluations_counts_every_enqueued_cycle_of_the_fp32_driver():
    """Three scripted cycles of restart 2; the third meets the tolerance after one inner step for both samples.  Lock step: every cycle has enqueued
    restart x precond_iterations evaluations whatever stopped on the way."""
    from helmnet_amd.gmres import drive_cycles, unet_evaluations
    t = lambda *rows: np.asarray(rows, np.float32)  # noqa: E731
    s = _Script([(t([1.0, 2.0], [0.5, 1.0], [0.2, 0.6]), [2, 2]), (t([0.2, 0.6], [0.1, 0.3], [0.05, 0.2]), [2, 2]),
                 (t([0.05, 0.2], [1e-5, 2e-5], [1e-5, 2e-5]), [1, 1])])
    out = drive_cycles(s.cycle, lambda: np.asarray([1e-5, 2e-5], np.float32), max_cycles=10, tol=1e-4)
    assert out["converged"] and out["cycles"] == 3 and s.calls == 3 and out["iterations"] == 5
    assert unet_evaluations(out["cycles"], 2, 5) == 30
    assert unet_evaluations(out["cycles"], 2, 0) == 0                    # no preconditioner: none
    assert unet_evaluations(0, 20, 5) == 0


def test_unet_evaluations_counts_the_checking_cycle_of_the_refinement():
    """The refinement's last call finds every sample below tol and updates nothing, but its launches ran: it counts."""
    from helmnet_amd.gmres import drive_refinement, unet_evaluations
    tab = [[1.0, 1.0], [0.1, 0.2], [0.01, 0.05]]
    s = _Script([([3e-2, 2e-2], tab, [2, 2]), ([4e-7, 1e-6], tab, [2, 2]), ([5e-11, 2e-11], [[1.0, 1.0]] * 3, [0, 0]), ([0.0, 0.0], tab, [0, 0])])
    out = drive_refinement(s.cycle, max_cycles=10, tol=1e-10)
    assert out["converged"] and out["cycles"] == 3 and s.calls == 3 and out["iterations"] == 4
    assert unet_evaluations(out["cycles"], 2, 3) == 18
    s = _Script([([1.0], [[1.0], [0.5], [0.25]], [2])] * 4)
    out = drive_refinement(s.cycle, max_cycles=4, tol=1e-10)             # not converged: the four cycles that ran
    assert not out["converged"] and unet_evaluations(out["cycles"], 2, 5) == 40


# ---------------------------------------------------------------------------------------------- the result dicts of gmres(backend="hip"), scripted engine
class _FakeEngine:
    """The engine calls of the two HIP drivers, answered from a script on the CPU; ``calls`` keeps (method, precond_iters, precond_scale)."""

    def __init__(self, script, true_rmse):
        self.script, self.true, self.calls = list(script), true_rmse, []

    def _next(self, name, m, alpha):
        self.calls.append((name, m, alpha))
        return self.script[len(self.calls) - 1]

    def gmres_cycle(self, x, k_sq, rhs, restart, tol, basis, hess):
        rm, ku = self._next("gmres_cycle", None, None)
        return torch.tensor(rm, dtype=torch.float32), torch.tensor(ku, dtype=torch.int32)

    def fgmres_cycle(self, x, k_sq, rhs, restart, tol, m, alpha, basis, hess, zbasis):
        assert tuple(zbasis.shape) == (x.shape[0], restart, basis.shape[-1]) and tuple(basis.shape) == (x.shape[0], restart + 1, basis.shape[-1])
        rm, ku = self._next("fgmres_cycle", m, alpha)
        return torch.tensor(rm, dtype=torch.float32), torch.tensor(ku, dtype=torch.int32)

    def gmres_refine_cycle(self, x, k_sq, rhs, restart, tol, floor, basis, hess):
        r64, rm, ku = self._next("gmres_refine_cycle", None, None)
        return torch.tensor(r64, dtype=torch.float64), torch.tensor(rm, dtype=torch.float32), torch.tensor(ku, dtype=torch.int32)

    def fgmres_refine_cycle(self, x, k_sq, rhs, restart, tol, m, alpha, floor, basis, hess, zbasis):
        assert tuple(zbasis.shape) == (x.shape[0], restart, basis.shape[-1]) and x.dtype == torch.float64
        r64, rm, ku = self._next("fgmres_refine_cycle", m, alpha)
        return torch.tensor(r64, dtype=torch.float64), torch.tensor(rm, dtype=torch.float32), torch.tensor(ku, dtype=torch.int32)

    def residual(self, x, k_sq, rhs):
        return x

    def rmse(self, res):
        return torch.tensor(self.true, dtype=torch.float32)

    def check_async_errors(self):
        pass


class _FakeSolver:
    def __init__(self, eng, n=4):
        self.eng, self.n = eng, n
        self.source = torch.zeros(1, 2, n, n)
        self.source[0, 0, 1, 2], self.source[0, 1, 1, 2] = 3.0, 4.0            # 2-norm 5

    def engine(self):
        return self.eng

    def get_initials(self, sos):
        return torch.ones(sos.shape[0], 1, self.n, self.n), torch.zeros(sos.shape[0], 2, self.n, self.n)


_FP32_SCRIPT = [([[1.0, 2.0], [0.5, 1.0], [0.2, 0.6]], [2, 2]), ([[0.2, 0.6], [0.1, 0.3], [0.05, 0.2]], [2, 2]),
                ([[0.05, 0.2], [1e-5, 2e-5], [1e-5, 2e-5]], [1, 1])]


def test_fp32_driver_result_carries_unet_evaluations_and_passes_the_preconditioner_on():
    from helmnet_amd.gmres import gmres
    sos = torch.ones(2, 1, 4, 4)
    eng = _FakeEngine(_FP32_SCRIPT, [1e-5, 2e-5])
    out = gmres(_FakeSolver(eng), sos, restart=2, max_outer=10, tol=1e-4, backend="hip", precondition="learned", precond_iterations=5)
    assert eng.calls == [("fgmres_cycle", 5, 5.0)] * 3                       # alpha: the default, the source's RMS 2-norm
    assert out["converged"] and len(out["cycle_tables"]) == 3 and out["iterations"] == 5
    assert out["unet_evaluations"] == 3 * 2 * 5
    assert out["operator_applications"] == 3 * 3 + 1                         # unchanged accounting: the cycles' and the one true check
    eng = _FakeEngine(_FP32_SCRIPT, [1e-5, 2e-5])
    out = gmres(_FakeSolver(eng), sos, restart=2, max_outer=2, tol=1e-4, backend="hip", precondition="learned", precond_iterations=1, precond_scale=0.25)
    assert eng.calls == [("fgmres_cycle", 1, 0.25)] * 2 and not out["converged"] and out["unet_evaluations"] == 2 * 2 * 1
    # no preconditioner: the plain cycle is what runs, and the count is zero; the keys of before are all there
    eng = _FakeEngine(_FP32_SCRIPT, [1e-5, 2e-5])
    out = gmres(_FakeSolver(eng), sos, restart=2, max_outer=10, tol=1e-4, backend="hip")
    assert eng.calls == [("gmres_cycle", None, None)] * 3 and out["unet_evaluations"] == 0
    assert {"wavefield", "residual_norms", "iterations", "operator_applications", "converged", "iterations_per_sample", "cycle_tables"} <= set(out)


def test_refined_driver_result_counts_the_checking_cycle():
    from helmnet_amd.gmres import gmres
    tab = [[1.0, 1.0], [0.1, 0.2], [0.01, 0.05]]
    script = [([3e-2, 2e-2], tab, [2, 2]), ([4e-7, 1e-6], tab, [2, 2]), ([5e-11, 2e-11], [[1.0, 1.0]] * 3, [0, 0])]
    sos = torch.ones(2, 1, 4, 4)
    eng = _FakeEngine(script, None)
    out = gmres(_FakeSolver(eng), sos, restart=2, max_outer=10, tol=1e-10, backend="hip", refine=True, precondition="learned", precond_iterations=3,
                precond_scale=2.0)
    assert eng.calls == [("fgmres_refine_cycle", 3, 2.0)] * 3
    assert out["converged"] and out["cycles"] == 3 and out["unet_evaluations"] == 3 * 2 * 3 and out["wavefield"].dtype == torch.float64
    assert out["residual_norm64"].tolist() == [5e-11, 2e-11]
    eng = _FakeEngine(script, None)
    out = gmres(_FakeSolver(eng), sos, restart=2, max_outer=10, tol=1e-10, backend="hip", refine=True)
    assert eng.calls == [("gmres_refine_cycle", None, None)] * 3 and out["unet_evaluations"] == 0 and out["cycles"] == 3
