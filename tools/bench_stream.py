"""Many maps to a tolerance: IterativeSolver.solve_many against the batch-wise solve_to_tolerance loop, and what the two stream launches cost.

    python tools/bench_stream.py [--tol 1e-4] [--max-iterations 1000] [--check-every 25] [--out profiles/stream_bench.txt]

The job is the 256-map set of BASELINE.json configs[2] (ring_sos_batch(256, 32, seed=r) for r in 0..7, source [30, 128], as tests/test_long_run.py builds
it).  Two GPU steps, each a child process under its own `timeout -k 10`, the second only if the first succeeded, nothing retried:
  solve    the job solved twice in one process -- solve_many(slots=32), then eight solve_to_tolerance batches of 32 (same tolerance, same check interval):
           wall time (host clock around work that ends in a synchronise, after a warm-up of every shape) and sample-iterations of both;
  launch   hn_stream_swap and hn_stream_verdict bracketed by device events at 256^2 x 32 -- all 32 slots turning over (the worst case) and 4 of them --
           against the time of one chunk of check_every iterations measured in the same process.
Run it once; the output file is indexed in profiles/README.md."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SLOTS, LOC = 256, 32, [30, 128]


def _solver():
    import torch
    sys.path.insert(0, ROOT)
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(torch.device("cuda:0"))
    s.set_domain_size(N, source_location=LOC)
    return s


def _job():
    import numpy as np
    import torch
    from helmnet_amd.phantoms import ring_sos_batch
    return torch.from_numpy(np.concatenate([ring_sos_batch(N, 32, seed=r) for r in range(8)])).to("cuda:0")


def step_solve(a):
    import torch
    s = _solver()
    sos = _job()
    # warm-up: allocations, tables, the side-stream probe, every batch size the tail of solve_many runs (a short job of 40 maps)
    s.solve_many(sos[:40], a.tol, max_iterations=2 * a.check_every, slots=SLOTS, check_every=a.check_every)
    s.solve_to_tolerance(sos[:SLOTS], a.tol, max_iterations=2 * a.check_every, check_every=a.check_every)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = s.solve_many(sos, a.tol, max_iterations=a.max_iterations, slots=SLOTS, check_every=a.check_every)
    torch.cuda.synchronize()
    t_stream = time.perf_counter() - t0
    t0 = time.perf_counter()
    batch_iters, worst = [], []
    for lo in range(0, sos.shape[0], SLOTS):
        o = s.solve_to_tolerance(sos[lo:lo + SLOTS], a.tol, max_iterations=a.max_iterations, check_every=a.check_every)
        batch_iters.append(int(o["iterations"]))
        worst.append(float(o["residual_norms"][-1].max()))
    torch.cuda.synchronize()
    t_batch = time.perf_counter() - t0
    it = out["iterations"]
    print(json.dumps({"step": "solve", "maps": int(sos.shape[0]), "domain": N, "slots": SLOTS, "tol": a.tol, "max_iterations": a.max_iterations,
                      "check_every": a.check_every,
                      "solve_many": {"seconds": round(t_stream, 4), "sample_iterations": out["sample_iterations"], "chunks": out["chunks"],
                                     "status_counts": [int((out["status"] == k).sum()) for k in (0, 1, 2)],
                                     "iterations_min_median_max": [int(it.min()), int(it.median()), int(it.max())],
                                     "ms_per_sample_iteration": round(t_stream / out["sample_iterations"] * 1e3, 5)},
                      "solve_to_tolerance_x8": {"seconds": round(t_batch, 4), "sample_iterations": SLOTS * sum(batch_iters),
                                                "iterations_per_batch": batch_iters, "worst_rmse_per_batch": worst,
                                                "ms_per_sample_iteration": round(t_batch / (SLOTS * sum(batch_iters)) * 1e3, 5)},
                      "wall_ratio_batchwise_over_stream": round(t_batch / t_stream, 3)}))


def step_launch(a):
    import numpy as np
    import torch
    s = _solver()
    eng = s.engine()
    sos = _job()[:64]
    dev = sos.device
    new = lambda *shape: torch.zeros(shape, device=dev)  # noqa: E731
    wf, res, st, ks = new(SLOTS, 2, N, N), new(SLOTS, 2, N, N), new(SLOTS, 2, eng.state_len), new(SLOTS, 1, N, N)
    out_wf, rmse, src = new(64, 2, N, N), new(a.check_every, SLOTS), s._src()
    eng.stream_swap(wf, res, st, ks, src, [(j, -1, -1, j) for j in range(SLOTS)], sos, None, 1.0, out_wf)
    # one chunk of the solver at this shape, for scale
    for _ in range(2):
        eng.step(wf, res, st, ks, src, a.check_every, rmse_hist=rmse)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 8
    for _ in range(reps):
        eng.step(wf, res, st, ks, src, a.check_every, rmse_hist=rmse)
    torch.cuda.synchronize()
    chunk_ms = (time.perf_counter() - t0) / reps * 1e3

    def bracket(fn, reps=20):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    turn = {k: [(j, j, -1, j + 32) for j in range(k)] for k in (32, 4)}     # slot j: retire map j, refill with map j + 32
    swap32 = bracket(lambda: eng.stream_swap(wf, res, st, ks, src, turn[32], sos, None, 1.0, out_wf))
    swap4 = bracket(lambda: eng.stream_swap(wf, res, st, ks, src, turn[4], sos, None, 1.0, out_wf))
    move4 = bracket(lambda: eng.stream_swap(wf, res, st, ks, src, [(j, j, 31 - j, -1) for j in range(4)], sos, None, 1.0, out_wf))
    verdict = bracket(lambda: eng.stream_verdict(rmse, a.tol))
    row_bytes = 4 * (6 * N * N + 2 * eng.state_len)       # wf, res, k_sq, sos planes + the state row: written (and read, for a retire / move) per slot
    print(json.dumps({"step": "launch", "domain": N, "slots": SLOTS, "check_every": a.check_every,
                      "chunk_ms": round(chunk_ms, 4), "ms_per_iteration": round(chunk_ms / a.check_every, 5),
                      "swap_32_slots_retire_refill_ms_median_min": [round(v, 4) for v in swap32],
                      "swap_4_slots_retire_refill_ms_median_min": [round(v, 4) for v in swap4],
                      "swap_4_slots_retire_move_ms_median_min": [round(v, 4) for v in move4],
                      "verdict_ms_median_min": [round(v, 4) for v in verdict],
                      "approx_bytes_written_per_slot": row_bytes,
                      "worst_case_share_of_chunk": round((swap32[0] + verdict[0]) / chunk_ms, 5),
                      "four_slot_share_of_chunk": round((swap4[0] + verdict[0]) / chunk_ms, 5)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--check-every", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.txt"))
    ap.add_argument("--step", choices=["solve", "launch"])
    a = ap.parse_args()
    if a.step:
        {"solve": step_solve, "launch": step_launch}[a.step](a)
        sys.exit(0)
    lines = [f"# python tools/bench_stream.py --tol {a.tol} --max-iterations {a.max_iterations} --check-every {a.check_every}"]
    passthrough = ["--tol", str(a.tol), "--max-iterations", str(a.max_iterations), "--check-every", str(a.check_every)]
    rc = 0
    for step, limit in (("solve", 300), ("launch", 120)):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + passthrough,
                           capture_output=True, text=True)
        if r.returncode != 0 or not r.stdout.strip():
            lines.append(f"# step {step} failed (exit {r.returncode}); later steps not started\n{r.stderr[-2000:]}")
            rc = r.returncode or 1
            break
        lines.append(r.stdout.strip().splitlines()[-1])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.exit(rc)
