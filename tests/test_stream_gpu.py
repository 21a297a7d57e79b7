"""IterativeSolver.solve_many on the GPU: per-sample stop, slot refill and tail compaction (hn_stream_verdict / hn_stream_swap).

Inputs and tolerances, chosen on the CPU from the float64 oracle before any GPU run:

  96^2   ring_sos_batch(96, 11, seed=31), source [82, 48], slots 8 (N = slots + 3).  ``oracle.solve`` in float64, 600 iterations per map:
         residual RMSE floors (minimum over the 600 iterations) 2.1e-5 .. 2.6e-5, the slowest map (#1) 3.9e-5 and still falling.
         tol = 2e-4 (5 x the slowest map's floor); the oracle's first iteration below it, per map:
             124 149 55 90 54 64 57 102 143 66 91        -> chunks of 25:  125 150 75 100 75 75 75 125 150 75 100
         and every trace stays below tol from its crossing on (at tol = 1e-4 map #1 crosses at 280 and is back above at 300: not used).
         max_iterations 400: the oracle converges on all 11 maps, none ends with status 1.
  256^2  the five maps of tests/golden/long_run.npz (cfg2: README map + ring_sos_batch(256, 4, seed=11), source [30, 128]), whose float64
         reference traces are committed (cfg2_rmse_f64, 1000 iterations): floors 1.3e-5 .. 2.0e-5.  tol = 1e-4 (5 x the slowest floor);
         first iteration below it:  112 438 120 111 98  -> chunks of 25:  125 450 125 125 100, monotone from the crossing on.
         The job is those five maps eight times over (N = 40 = slots + 8, slots 32): every slot route of a full batch, refills and the tail.
         max_iterations 1000: none ends with status 1.

hn_step's per-sample RMSE rows are sums of float atomics (tests/test_long_run.py:251 compares them with rtol 1e-5), so ``residual_norm`` is compared
with that bar; wavefields and residuals are compared bit for bit.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_inputs import long_inputs
from helmnet_amd.phantoms import ring_sos_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {
    96: dict(loc=[82, 48], slots=8, tol=2e-4, max_iterations=400, oracle=[124, 149, 55, 90, 54, 64, 57, 102, 143, 66, 91]),
    256: dict(loc=[30, 128], slots=32, tol=1e-4, max_iterations=1000, oracle=[112, 438, 120, 111, 98] * 8),
}
CHECK_EVERY = 25


def _solver(n, loc, precision=None):
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    if precision is not None:
        s.set_unet_precision(precision)
    s.set_domain_size(n, source_location=loc)
    return s


def _maps(n):
    if n == 96:
        return torch.from_numpy(ring_sos_batch(96, 11, seed=31)).to(DEV)
    return torch.from_numpy(np.concatenate([long_inputs("cfg2")["sos"]] * 8)).to(DEV)


_JOBS = {}


def _job(n):
    """solve_many on the set of size n (once per session) and every DISTINCT map solved alone by forward() for the iterations solve_many reports."""
    if n not in _JOBS:
        cfg, sos = SETS[n], _maps(n)
        s = _solver(n, cfg["loc"])
        out = s.solve_many(sos, cfg["tol"], max_iterations=cfg["max_iterations"], slots=cfg["slots"], check_every=CHECK_EVERY, keep_residuals=True)
        torch.cuda.synchronize()
        print(f"[stream {n}] iterations {out['iterations'].tolist()} (oracle first-below {cfg['oracle']}) status {out['status'].tolist()} "
              f"sample_iterations {out['sample_iterations']} chunks {out['chunks']}")
        print(f"[stream {n}] residual_norm {[f'{v:.3e}' for v in out['residual_norm'].tolist()]}")
        alone = {}
        distinct = range(sos.shape[0]) if n == 96 else range(5)
        for m in distinct:
            o = s.forward(sos[m:m + 1], num_iterations=int(out["iterations"][m]), residuals="norms")
            alone[m] = (o["wavefields"][0][0].clone(), o["last_residual"][0].clone(), float(o["residual_norms"][-1, 0]))
        _JOBS[n] = (cfg, sos, s, out, alone)
    return _JOBS[n]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("per_map_sources", [False, True], ids=["shared_source", "per_map_sources"])
@pytest.mark.parametrize("n", [96, 256, 272])
def test_refill_equals_the_start_of_forward(n, per_map_sources):
    loc = {96: [82, 48], 256: [30, 128], 272: [40, 136]}[n]
    s = _solver(n, loc)
    sos = torch.from_numpy(ring_sos_batch(n, 3, seed=5)).to(DEV)
    if per_map_sources:
        s.set_multiple_sources([loc, [loc[0] + 7, loc[1] - 9], [n // 2, n // 2]])
    eng = s.engine()
    k_sq, wf0 = s.get_initials(sos)
    s.f.clear_states(wf0)
    res0 = s.get_residual(wf0, k_sq)
    st0 = s.f.get_states(flatten=True).contiguous()
    assert float(res0.abs().max()) > 0
    slots, junk = 4, 7.25
    full = lambda *shape: torch.full(shape, junk, device=DEV)  # noqa: E731
    wf, res, st, ks = full(slots, 2, n, n), full(slots, 2, n, n), full(slots, 2, eng.state_len), full(slots, 1, n, n)
    src_in = s.source.detach().float().clone().contiguous() if per_map_sources else None
    src = full(slots, 2, n, n) if per_map_sources else s._src()
    where = [2, 0, 3]                                                       # map m goes to slot where[m]; slot 1 is left alone
    eng.stream_swap(wf, res, st, ks, src, [(where[m], -1, -1, m) for m in range(3)], sos, src_in, float(s.hparams.omega))
    torch.cuda.synchronize()
    for m, slot in enumerate(where):
        for got, want, name in ((ks[slot], k_sq[m], "k_sq"), (wf[slot], wf0[m], "wf"), (res[slot], res0[m], "res"), (st[slot], st0[m], "states")):
            assert torch.equal(got, want), (name, m)
            assert torch.equal(_bits(got), _bits(want)), (name, m, "signed zeros")
        if per_map_sources:
            assert torch.equal(src[slot], src_in[m])
    for t in (wf, res, st, ks) + ((src,) if per_map_sources else ()):
        assert bool((t[1] == junk).all())
    # another omega: the kernel's k_sq is torch's `(omega / sos) ** 2` in fp32, bit for bit
    eng.stream_swap(wf, res, st, ks, src, [(1, -1, -1, 2)], sos, src_in, 1.7)
    torch.cuda.synchronize()
    assert torch.equal(ks[1], (1.7 / sos[2]) ** 2)


# ---------------------------------------------------------------------------------------------------------------- 2, 5
@pytest.mark.parametrize("n", [96, 256])
def test_every_map_is_bit_identical_to_forward_alone(n):
    cfg, sos, s, out, alone = _job(n)
    N = sos.shape[0]
    assert out["wavefields"].shape == (N, 2, n, n) and out["residuals"].shape == (N, 2, n, n)
    assert out["iterations"].dtype == torch.int64 and out["status"].dtype == torch.int8 and out["residual_norm"].shape == (N,)
    assert cfg["slots"] <= 32                     # a statement about routes: beyond 32 maps per call the deep kernel is bypassed
    for m in range(N):
        ref = m if n == 96 else m % 5
        if ref != m:
            assert int(out["iterations"][m]) == int(out["iterations"][ref]), (m, ref)
        wf, res, norm = alone[ref]
        assert torch.equal(out["wavefields"][m], wf), (n, m, int(out["iterations"][m]), float((out["wavefields"][m] - wf).abs().max()))
        assert torch.equal(out["residuals"][m], res), (n, m)
        assert abs(float(out["residual_norm"][m]) / norm - 1) <= 1e-5, (n, m, float(out["residual_norm"][m]), norm)


@pytest.mark.parametrize("n", [96, 256])
def test_tail_compaction_runs_a_shrinking_dense_prefix(n):
    """N = slots + 3 (96^2) / slots + 8 (256^2): once the maps run out the last chunks run with fewer active slots than ``slots`` -- the work enqueued is
    then less than slots x iterations of all chunks -- and the results of those chunks are the bit-identical ones of the test above."""
    cfg, sos, s, out, alone = _job(n)
    assert sos.shape[0] > cfg["slots"]
    assert cfg["max_iterations"] % CHECK_EVERY == 0                         # so every chunk is CHECK_EVERY long
    assert out["sample_iterations"] < cfg["slots"] * CHECK_EVERY * out["chunks"]
    assert out["sample_iterations"] == int(out["iterations"].sum())


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("n", [96, 256])
def test_every_status_is_right(n):
    cfg, sos, s, out, alone = _job(n)
    it, status, norm = out["iterations"].numpy(), out["status"].numpy(), out["residual_norm"].cpu().numpy()
    assert set(status.tolist()) <= {0, 1}
    assert (status == 1).sum() <= 1, status
    assert (norm[status == 0] < cfg["tol"]).all(), norm
    assert (it[status == 1] == cfg["max_iterations"]).all() and (norm[status == 1] >= cfg["tol"]).all()
    assert (it % CHECK_EVERY == 0).all() and (it >= CHECK_EVERY).all() and (it <= cfg["max_iterations"]).all()
    assert torch.isfinite(out["wavefields"]).all()


def test_a_map_with_a_nan_pixel_is_retired_after_its_first_chunk_and_disturbs_nobody():
    cfg, sos, s, out, alone = _job(96)
    bad = sos.clone()
    bad[4, 0, 40, 50] = float("nan")           # NaN as data: k_sq is NaN there, the residual norm NaN after one iteration
    o = s.solve_many(bad, cfg["tol"], max_iterations=cfg["max_iterations"], slots=cfg["slots"], check_every=CHECK_EVERY)
    assert int(o["status"][4]) == 2 and int(o["iterations"][4]) == CHECK_EVERY
    keep = [m for m in range(sos.shape[0]) if m != 4]
    assert torch.equal(o["status"][keep], out["status"][keep]) and torch.equal(o["iterations"][keep], out["iterations"][keep])
    assert torch.equal(o["wavefields"][keep], out["wavefields"][keep])
    # a bound on the RMSE instead: 1e-30 is exceeded by every map in its first chunk
    o = s.solve_many(sos[:3], cfg["tol"], max_iterations=cfg["max_iterations"], slots=2, check_every=CHECK_EVERY, diverge_rmse=1e-30)
    assert o["status"].tolist() == [2, 2, 2] and o["iterations"].tolist() == [CHECK_EVERY] * 3


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("n", [96, 256])
def test_less_work_than_the_batch_wise_loop(n):
    cfg, sos, s, out, alone = _job(n)
    batchwise = 0
    for lo in range(0, sos.shape[0], cfg["slots"]):
        part = sos[lo:lo + cfg["slots"]]
        o = s.solve_to_tolerance(part, cfg["tol"], max_iterations=cfg["max_iterations"], check_every=CHECK_EVERY)
        batchwise += part.shape[0] * int(o["iterations"])       # (the last batch counted with its own size, not with `slots`: the stricter comparison)
    print(f"[stream {n}] sample-iterations: solve_many {out['sample_iterations']}, batch-wise solve_to_tolerance {batchwise}")
    assert out["sample_iterations"] < batchwise
    assert out["sample_iterations"] == int(out["iterations"].sum())     # every chunk is full here: no tail-chunk remainder


# ---------------------------------------------------------------------------------------------------------------- 6
def test_refusals():
    from helmnet_amd._lib import HelmnetHipError
    n, slots = 64, 4
    s = _solver(n, [20, 32])
    eng = s.engine()
    sos = torch.from_numpy(ring_sos_batch(n, 6, seed=2)).to(DEV)
    junk = 3.5
    full = lambda *shape: torch.full(shape, junk, device=DEV)  # noqa: E731
    wf, res, st, ks = full(slots, 2, n, n), full(slots, 2, n, n), full(slots, 2, eng.state_len), full(slots, 1, n, n)
    src, out_wf = s._src(), full(6, 2, n, n)
    rmse = full(5, slots)
    arrays = (wf, res, st, ks, out_wf)

    def swap(ops, **kw):
        eng.stream_swap(wf, res, st, ks, kw.get("src", src), ops, sos, kw.get("src_in"), 1.0, out_wf)

    for ops in ([(0, -1, -1, 0), (0, -1, -1, 1)],                # a slot named twice
                [(0, -1, 1, -1), (1, -1, -1, 0)],                # a move that reads a slot the same call refills
                [(0, -1, 1, -1), (1, -1, 2, -1)],                # ... or moves into
                [(0, -1, 0, -1)],                                # a move onto itself
                [(slots, -1, -1, 0)], [(-1, -1, -1, 0)],         # slot out of range
                [(0, -1, -1, 6)], [(0, 6, -1, -1)], [(0, -2, -1, -1)],   # map out of range
                [(0, 3, -1, -1), (1, 3, -1, -1)],                # a map retired twice
                [(0, -1, slots, -1)]):                           # move_from out of range
        with pytest.raises(ValueError):
            swap(ops)
    with pytest.raises(ValueError):                              # src_batch neither 1 nor batch
        swap([(0, -1, -1, 0)], src=full(2, 2, n, n))
    with pytest.raises(ValueError):                              # one source row per slot but no per-map sources to refill from
        swap([(0, -1, -1, 0)], src=full(slots, 2, n, n))
    torch.cuda.synchronize()
    for t in arrays:
        assert bool((t == junk).all())                           # nothing was enqueued by a refused call

    # stream capture: HN_ERR_STATE before anything is enqueued -- the capture stays active and ends as an empty graph
    hip = ctypes.CDLL("libamdhip64.so")
    side = torch.cuda.Stream()
    handle = ctypes.c_void_p(side.cuda_stream)
    ops = np.asarray([(0, -1, -1, 0)], np.int32)
    graph, status, n_nodes = ctypes.c_void_p(), ctypes.c_int(-1), ctypes.c_size_t(99)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert hip.hipStreamBeginCapture(handle, 1) == 0         # hipStreamCaptureModeThreadLocal
        try:
            with pytest.raises(HelmnetHipError, match="status -2"):
                eng.stream_swap(wf, res, st, ks, src, ops, sos, None, 1.0, out_wf)
            with pytest.raises(HelmnetHipError, match="status -2"):
                eng.stream_verdict(rmse, 1e-3)
            assert hip.hipStreamIsCapturing(handle, ctypes.byref(status)) == 0
        finally:
            rc_end = hip.hipStreamEndCapture(handle, ctypes.byref(graph))
    assert status.value == 1                                     # hipStreamCaptureStatusActive
    assert rc_end == 0 and graph.value
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n_nodes)) == 0 and n_nodes.value == 0
    assert hip.hipGraphDestroy(graph) == 0
    torch.cuda.synchronize()
    for t in arrays:
        assert bool((t == junk).all())
    # the same calls work once the capture is over
    eng.stream_swap(wf, res, st, ks, src, ops, sos, None, 1.0, out_wf)
    table = eng.stream_verdict(rmse, 10.0)
    torch.cuda.synchronize()
    eng.check_async_errors()
    assert table["first_below"].tolist() == [0] * slots and table["bad"].tolist() == [0] * slots and table["last_rmse"].tolist() == [junk] * slots
    assert bool((wf[0] == 0).all()) and bool((wf[1:] == junk).all())

    # solve_many is the no-grad path
    with pytest.raises(RuntimeError):
        s.solve_many(sos.clone().requires_grad_(True), 1e-3, max_iterations=50)
    with pytest.raises(ValueError):
        s.solve_many(sos[:, :, :32], 1e-3, max_iterations=50)
    # an empty job
    o = s.solve_many(sos[:0], 1e-3, max_iterations=50)
    assert o["wavefields"].shape == (0, 2, n, n) and o["iterations"].numel() == 0 and o["sample_iterations"] == 0


def test_verdict_records():
    """first_below / bad / last_rmse from a hand-made RMSE table, NaN and Inf rows and the divergence bound included."""
    s = _solver(64, [20, 32])
    eng = s.engine()
    rows = torch.tensor([[5e-3, 5e-3, 5e-3, 5e-3, 5e-3],
                         [9e-4, 2e-3, float("nan"), 2e-3, 2e-3],
                         [2e-3, 1e-3, 1e-4, float("inf"), 0.5],
                         [8e-4, 1.5e-3, 1e-4, 1e-4, 1e-4]], device=DEV)
    t = eng.stream_verdict(rows, 1e-3)
    torch.cuda.synchronize()
    assert t["first_below"].tolist() == [1, -1, 2, 3, 3] and t["bad"].tolist() == [0, 0, 1, 1, 0]
    assert np.array_equal(t["last_rmse"], rows[-1].cpu().numpy())
    t = eng.stream_verdict(rows, 1e-3, diverge_rmse=0.1)
    torch.cuda.synchronize()
    assert t["bad"].tolist() == [0, 0, 1, 1, 1]


# ---------------------------------------------------------------------------------------------------------------- 7, per-map sources
def test_fp16_unet_mode():
    cfg, sos = SETS[96], _maps(96)
    s = _solver(96, cfg["loc"], precision="fp16")
    out = s.solve_many(sos, cfg["tol"], max_iterations=cfg["max_iterations"], slots=cfg["slots"], check_every=CHECK_EVERY)
    assert s.engine().unet_precision == "fp16"
    print(f"[stream fp16] iterations {out['iterations'].tolist()} status {out['status'].tolist()}")
    assert set(out["status"].tolist()) <= {0, 1}
    assert torch.isfinite(out["wavefields"]).all() and torch.isfinite(out["residual_norm"]).all()
    # no bit-identity is claimed in this mode; the comparison with forward() alone is printed, not asserted (it has not been measured)
    for m in (0, 1, 9):
        o = s.forward(sos[m:m + 1], num_iterations=int(out["iterations"][m]), residuals="norms")
        d = float((out["wavefields"][m] - o["wavefields"][0][0]).abs().max())
        print(f"[stream fp16] map {m}: Linf(solve_many - forward alone) = {d:.3e}")


def test_per_map_sources_follow_their_maps_through_refill_and_compaction():
    n, loc = 96, [82, 48]
    sos = _maps(96)[:7]
    s = _solver(n, loc)
    locs = [[82, 48], [80, 40], [78, 56], [82, 48], [70, 48], [82, 60], [76, 44]]
    s.set_multiple_sources(locs)
    sources = s.source.detach().float().clone()
    s.set_multiple_sources([loc])
    out = s.solve_many(sos, 2e-4, max_iterations=200, slots=3, check_every=CHECK_EVERY, source_maps=sources)
    assert set(out["status"].tolist()) <= {0, 1}
    for m in range(7):
        s.set_source_maps(sources[m:m + 1].clone())
        o = s.forward(sos[m:m + 1], num_iterations=int(out["iterations"][m]), residuals="norms")
        assert torch.equal(out["wavefields"][m], o["wavefields"][0][0]), m
