#!/usr/bin/env python
"""Seconds per inner GMRES(20) iteration for both backends of helmnet_amd.gmres, in one process with alternating runs.

    python tools/bench_gmres.py [--out FILE]

Shapes 256^2 x 4 and 256^2 x 32.  Cycles run with tol = 0 (every inner step, no early exit).  Also: the operator alone (hn_residual), and the
floor of an average step -- its basis traffic divided by the copy bandwidth measured here (a device-to-device copy of a basis-sized buffer).
Times are medians of `--rounds` alternating rounds; the clock is the device's clock rate as torch reports it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from helmnet_amd import IterativeSolver
    from helmnet_amd.gmres import gmres
    from helmnet_amd.phantoms import ring_sos_batch
    dev, n, m = "cuda:0", 256, a.restart
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(dev)
    s.set_domain_size(n, source_location=[n - 62, n // 2])
    eng = s.engine()
    rows = []
    for batch in (4, 32):
        sos = torch.from_numpy(ring_sos_batch(n, batch, seed=11)).to(dev)
        k_sq = s.get_initials(sos)[0].contiguous()
        src = s.source.detach().float().contiguous()
        run = {b: (lambda b=b: gmres(s, sos, restart=m, max_outer=a.cycles, tol=0.0, backend=b)) for b in ("torch", "hip")}
        for b in run:
            run[b]()                                   # warm: workspace, kernels
        t = {"torch": [], "hip": []}
        for _ in range(a.rounds):
            for b in ("torch", "hip"):
                t[b].append(_timed(run[b]) / (a.cycles * m))
        wf = torch.randn(batch, 2, n, n, device=dev)
        reps = 200
        t_op = min(_timed(lambda: [eng.residual(wf, k_sq, src) for _ in range(reps)]) / reps for _ in range(3))
        buf = torch.empty(batch, m + 1, 2 * n * n, device=dev)
        dst = torch.empty_like(buf)
        t_cp = min(_timed(lambda: dst.copy_(buf)) for _ in range(5))
        bw = 2 * buf.numel() * 4 / t_cp                                   # bytes read + written per second
        # an average step (k = m / 2) reads the k + 1 basis vectors three times (two projections that also subtract share a pass: dots, subtract + dots,
        # subtract) and moves w / v a handful of times
        avg_bytes = (3 * (m / 2 + 1) + 8) * batch * 2 * n * n * 4
        rows.append({"shape": f"{n}x{n} x {batch}", "restart": m, "torch_s_per_inner_iteration": statistics.median(t["torch"]),
                     "hip_s_per_inner_iteration": statistics.median(t["hip"]), "speedup": statistics.median(t["torch"]) / statistics.median(t["hip"]),
                     "operator_only_s": t_op, "copy_bandwidth_GBps": bw / 1e9, "basis_traffic_bytes_avg_step": avg_bytes, "bandwidth_floor_s": avg_bytes / bw})
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "clock_rate_khz": getattr(props, "clock_rate", None), "cycles_per_run": a.cycles, "rounds": a.rounds, "rows": rows}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
