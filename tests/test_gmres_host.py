"""GMRES in the library, the part that needs no GPU: hn_gmres_cycle is declared, exported and bound; the host loop that turns per-cycle tables
into a history is exercised with a scripted cycle; the refusals of ``gmres`` that come before any GPU work."""
import os
import re
from ctypes import c_float, c_int, c_void_p

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_hn_gmres_cycle():
    from helmnet_amd import _lib
    from helmnet_amd.build import SOURCES, build
    build()
    lib = _lib.load()
    assert "hn_krylov.hip" in SOURCES
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    m = re.search(r"int hn_gmres_cycle\((.*?)\);", hdr, re.S)
    assert m, "hn_gmres_cycle is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.SYMBOLS["hn_gmres_cycle"]
    assert res is c_int and len(args) == len(params) == 13
    for p, a in zip(params, args):
        want = c_void_p if "*" in p else c_float if p.startswith("float ") else c_int
        assert a is want, (p, a)
    assert "spectral_gmres_solver.m:86-115" in hdr
    assert lib.hn_abi_version() == _lib.ABI_VERSION == 7      # a new entry point within ABI 7
    assert lib.hn_gmres_cycle(None, None, None, None, 1, 1, 1, 0.0, None, None, None, None, None) == -1


class _Script:
    """A scripted cycle: per cycle a (table [m + 1, B], k_used [B]) pair, then the true RMSE values handed out one per check."""

    def __init__(self, cycles, trues):
        self.cycles, self.trues, self.calls, self.checks = list(cycles), list(trues), 0, 0

    def cycle(self):
        out = self.cycles[self.calls]
        self.calls += 1
        return np.asarray(out[0], np.float32), np.asarray(out[1])

    def true_rmse(self):
        out = self.trues[self.checks]
        self.checks += 1
        return np.asarray(out, np.float32)


def test_driver_concatenates_histories_up_to_each_samples_k_used():
    from helmnet_amd.gmres import drive_cycles
    tol = 0.1
    # cycle 1 (restart 3): sample 0 runs all 3 steps, sample 1 all 3; nobody below tol -> no true check
    t1 = [[8.0, 4.0], [4.0, 3.0], [2.0, 2.5], [1.0, 2.0]]
    # cycle 2: sample 0 stops after 1 step (0.05 < tol), its later rows hold garbage the driver must not report; sample 1 stops after 3 (0.09)
    t2 = [[1.0, 2.0], [0.05, 1.0], [77.0, 0.5], [77.0, 0.09]]
    s = _Script([(t1, [3, 3]), (t2, [1, 3])], [[0.06, 0.08]])
    out = drive_cycles(s.cycle, s.true_rmse, max_cycles=10, tol=tol)
    assert out["converged"] and out["cycles"] == 2 and s.calls == 2 and s.checks == 1 and out["true_checks"] == 1
    assert out["iterations_per_sample"].dtype == np.int64 and out["iterations_per_sample"].tolist() == [4, 6]
    assert out["iterations"] == 6
    h = np.stack(out["history"])
    assert h.dtype == np.float32 and h.shape == (8, 2)
    want = np.array(t1 + [[1.0, 2.0], [0.05, 1.0], [0.05, 0.5], [0.06, 0.08]], np.float32)   # the last row is the true residual
    assert np.array_equal(h, want)
    assert len(out["tables"]) == 2 and np.array_equal(out["tables"][1], np.asarray(t2, np.float32))


def test_driver_sample_already_below_tol_contributes_zero():
    from helmnet_amd.gmres import drive_cycles
    t = [[0.01, 5.0], [0.01, 1.0], [0.01, 0.05]]
    s = _Script([(t, [0, 2])], [[0.01, 0.04]])
    out = drive_cycles(s.cycle, s.true_rmse, max_cycles=5, tol=0.1)
    assert out["converged"] and out["iterations_per_sample"].tolist() == [0, 2] and out["iterations"] == 2
    assert np.array_equal(np.stack(out["history"]), np.array([[0.01, 5.0], [0.01, 1.0], [0.01, 0.04]], np.float32))
    # every sample below tol at the start: one cycle call, no inner iteration, one history row
    s = _Script([([[0.01, 0.02], [0.01, 0.02]], [0, 0])], [[0.01, 0.02]])
    out = drive_cycles(s.cycle, s.true_rmse, max_cycles=5, tol=0.1)
    assert out["converged"] and out["iterations"] == 0 and len(out["history"]) == 1 and out["iterations_per_sample"].tolist() == [0, 0]


def test_driver_true_residual_above_tol_starts_another_cycle():
    from helmnet_amd.gmres import drive_cycles
    t1 = [[1.0], [0.05]]
    t2 = [[0.2], [0.04]]
    s = _Script([(t1, [1]), (t2, [1])], [[0.2], [0.03]])
    out = drive_cycles(s.cycle, s.true_rmse, max_cycles=5, tol=0.1)
    assert out["converged"] and out["cycles"] == 2 and out["true_checks"] == 2
    assert np.array_equal(np.stack(out["history"])[:, 0], np.array([1.0, 0.2, 0.2, 0.03], np.float32))


def test_driver_not_converged_when_max_cycles_runs_out():
    from helmnet_amd.gmres import drive_cycles
    t = [[4.0, 4.0], [3.0, 3.5], [2.0, 3.0]]
    s = _Script([(t, [2, 2])] * 3, [])
    out = drive_cycles(s.cycle, s.true_rmse, max_cycles=3, tol=0.1)
    assert not out["converged"] and out["cycles"] == 3 and s.calls == 3 and s.checks == 0
    assert out["iterations"] == 6 and out["iterations_per_sample"].tolist() == [6, 6] and len(out["history"]) == 9


def test_gmres_refusals_before_any_gpu_work():
    from helmnet_amd.gmres import gmres
    sos = torch.ones(1, 1, 16, 16)
    with pytest.raises(ValueError, match="nonsense"):
        gmres(None, sos, backend="nonsense")
    with pytest.raises(RuntimeError, match="grad"):
        gmres(None, sos.clone().requires_grad_(True), backend="hip")
    with pytest.raises(RuntimeError, match="grad"):
        gmres(None, sos, x0=torch.zeros(1, 2, 16, 16, requires_grad=True), backend="hip")
