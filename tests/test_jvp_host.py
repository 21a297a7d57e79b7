"""CPU-only checks of the forward-mode plumbing: the hn_step_jvp declaration and binding, the Python surface, the initial-tangent formulas and the
chunk driver of IterativeSolver.jvp (against a stub engine)."""
import os
import re

import torch
import torch.autograd.forward_ad as fwAD

from helmnet_amd import _lib
from oracle import helmnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_hn_step_jvp_and_lib_binds_it():
    hdr = open(os.path.join(ROOT, "include", "helmnet_hip.h")).read()
    m = re.search(r"int hn_step_jvp\((.*?)\);", hdr, re.S)
    assert m, "hn_step_jvp is not declared"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SYMBOLS["hn_step_jvp"]
    assert res is _lib.c_int
    # ctx, four inputs, three ints, the three tape histories, three in/out tangents, two input directions, three tangent histories, the stream
    assert len(params) == len(args) == 20
    for p, a in zip(params, args):
        assert (a is _lib.c_int) == (p.startswith("int ")), (p, a)
        assert (a is _lib.c_void_p) == ("*" in p), (p, a)
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["ctx", "wf0", "res0", "states0", "k_sq", "src_batch", "batch", "n_iter", "wf_hist", "res_hist", "st_hist", "t_wf", "t_res", "t_states",
                     "t_k_sq", "t_src", "t_wf_hist", "t_res_hist", "t_st_hist", "stream"]
    written = {n for p, n in zip(params, names) if "*" in p and not p.startswith("const ") and n not in ("ctx", "stream")}
    assert written == {"t_wf", "t_res", "t_states", "t_wf_hist", "t_res_hist", "t_st_hist"}
    assert re.search(r"#define HN_ABI_VERSION 7\b", hdr)
    build_py = open(os.path.join(ROOT, "helmnet_amd", "build.py")).read()
    assert '"hn_jvp.hip"' in build_py


def test_python_surface_exists():
    from helmnet_amd import IterativeSolver
    from helmnet_amd.autograd import Laplacian, Residual, Solve
    from helmnet_amd.engine import Engine
    assert callable(getattr(Engine, "step_jvp"))
    for fn in (Laplacian, Residual, Solve):
        assert "jvp" in vars(fn) and isinstance(vars(fn)["jvp"], staticmethod), fn
    assert callable(getattr(IterativeSolver, "jvp")) and callable(getattr(IterativeSolver, "linearize"))


def test_initial_tangents_match_forward_ad_of_the_oracle():
    from helmnet_amd.solver import jvp_initial_tangents
    n, b, omega = 16, 2, 1.3
    g = torch.Generator().manual_seed(3)
    sos = 1.0 + torch.rand(b, 1, n, n, generator=g, dtype=torch.float64)
    d_sos = torch.randn(b, 1, n, n, generator=g, dtype=torch.float64)
    src = torch.randn(1, 2, n, n, generator=g, dtype=torch.float64)
    d_src = torch.randn(1, 2, n, n, generator=g, dtype=torch.float64)
    tab = O.SpectralTables(n, 8, 2, 1.0, dtype=torch.float64)
    with fwAD.dual_level():
        k_sq, wf = O.get_initials(fwAD.make_dual(sos, d_sos), omega)
        res = O.get_residual(wf, k_sq, fwAD.make_dual(src, d_src), tab)
        want_k = fwAD.unpack_dual(k_sq).tangent.clone()
        want_res = fwAD.unpack_dual(res).tangent.clone()
        assert fwAD.unpack_dual(wf).tangent is None
    t_k, t_wf, t_res = jvp_initial_tangents(omega, sos, d_sos, d_src)
    assert float((t_k - want_k).abs().max() / want_k.abs().max()) <= 1e-14
    assert t_res.shape == (b, 2, n, n) and float((t_res - want_res).abs().max()) <= 1e-14 * float(want_res.abs().max())
    assert t_wf.shape == (b, 2, n, n) and not t_wf.any()
    t_k, t_wf, t_res = jvp_initial_tangents(omega, sos, None, None)
    assert t_k is None and not t_wf.any() and not t_res.any() and t_res.data_ptr() != t_wf.data_ptr()


class _StubEngine:
    """step: iteration i (counted over the whole solve) writes the value i + 1 everywhere; step_jvp records what it is handed."""

    def __init__(self):
        self.done, self.calls = 0, []

    def step(self, wf, res, st, k_sq, src, n_iter, res_hist, wf_hist, st_hist, rmse_hist):
        assert wf_hist.shape[0] == res_hist.shape[0] == st_hist.shape[0] == rmse_hist.shape[0] == n_iter
        for i in range(n_iter):
            self.done += 1
            for live, hist in ((wf, wf_hist), (res, res_hist), (st, st_hist)):
                live.fill_(self.done)
                hist[i] = live
            rmse_hist[i] = 100 + self.done

    def step_jvp(self, wf0, res0, st0, k_sq, src_batch, wf_hist, res_hist, st_hist, t_wf, t_res, t_st, t_k, t_src, *hist):
        assert not hist
        self.calls.append(dict(start=(float(wf0.flatten()[0]), float(res0.flatten()[0]), float(st0.flatten()[0])), src_batch=src_batch,
                               slots=[float(h.flatten()[0]) for h in wf_hist], n=(wf_hist.shape[0], res_hist.shape[0], st_hist.shape[0]),
                               same=bool((wf_hist[:, 0, 0, 0, 0] == res_hist[:, 0, 0, 0, 0]).all() and (wf_hist[:, 0, 0, 0, 0] == st_hist[:, 0, 0, 0]).all()),
                               t_in=float(t_wf.flatten()[0]), t_k=t_k, t_src=t_src))
        for t in (t_wf, t_res, t_st):
            t.add_(wf_hist.shape[0])


def test_chunk_driver_hands_each_chunk_its_slots_and_its_start():
    from helmnet_amd.solver import jvp_chunks
    b, n, L, K, chunk = 2, 4, 21, 10, 4
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    wf, res, st, k_sq, src = z(b, 2, n, n), z(b, 2, n, n), z(b, 2, L), z(b, 1, n, n), z(1, 2, n, n)
    t_wf, t_res, t_st, t_k = z(b, 2, n, n), z(b, 2, n, n), z(b, 2, L), z(b, 1, n, n)
    eng = _StubEngine()
    rmse = jvp_chunks(eng, wf, res, st, k_sq, src, t_wf, t_res, t_st, t_k, None, K, chunk)
    assert [c["n"] for c in eng.calls] == [(4, 4, 4), (4, 4, 4), (2, 2, 2)]
    assert [c["slots"] for c in eng.calls] == [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10]]
    assert [c["start"] for c in eng.calls] == [(0, 0, 0), (4, 4, 4), (8, 8, 8)]       # the state in front of each chunk, not the one behind it
    assert [c["t_in"] for c in eng.calls] == [0, 4, 8]                                  # the tangents are carried from chunk to chunk
    assert all(c["same"] and c["src_batch"] == 1 and c["t_k"] is t_k and c["t_src"] is None for c in eng.calls)
    assert float(wf.flatten()[0]) == K and float(t_wf.flatten()[0]) == K and rmse.tolist() == [100 + K] * b
    eng = _StubEngine()                                                                  # a chunk larger than the solve: one call
    jvp_chunks(eng, z(b, 2, n, n), z(b, 2, n, n), z(b, 2, L), k_sq, src, z(b, 2, n, n), z(b, 2, n, n), z(b, 2, L), None, None, 3, 25)
    assert [c["slots"] for c in eng.calls] == [[1, 2, 3]]
