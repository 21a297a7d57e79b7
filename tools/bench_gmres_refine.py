#!/usr/bin/env python
"""Seconds per restart cycle of GMRES(20): the plain fp32 cycle (hn_gmres_cycle) next to the refined one (hn_gmres_refine_cycle: the same cycle plus
one float64 operator application and three streaming launches), in one process with alternating runs.

    python tools/bench_gmres_refine.py [--f64-fft 0] [--out FILE]

Shapes 256^2 x 4 and 256^2 x 32, as tools/bench_gmres.py.  Both run every inner step (tol = 0, inner_floor = 0) and are enqueued back to back, `--cycles`
calls per timed window with one synchronisation at its end (no host read-back: the driver's one read per cycle is not part of either figure).  Also:
the float64 operator alone (hn_residual_f64 with its RMSE), on the route --f64-fft picks (option 'f64_fft': 0 dense, 1 FFT).  Times are medians of `--rounds` alternating rounds; the shader clock is the median of the
board's hwmon readings while the timed windows run (bench.py's sampler), null where the board does not expose it."""
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
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--f64-fft", type=int, default=0, choices=(0, 1), help="route of the float64 operator (option 'f64_fft')")
    a = ap.parse_args()
    from bench import Hwmon
    from helmnet_amd import IterativeSolver
    from helmnet_amd.phantoms import ring_sos_batch
    dev, n, m = "cuda:0", 256, a.restart
    s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(dev)
    s.set_domain_size(n, source_location=[n - 62, n // 2])
    eng = s.engine()
    eng.set_option("f64_fft", a.f64_fft)
    rows = []
    hw = Hwmon(torch.device(dev))
    with hw:
        for batch in (4, 32):
            sos = torch.from_numpy(ring_sos_batch(n, batch, seed=11)).to(dev)
            k_sq = s.get_initials(sos)[0].contiguous()
            src = s.source.detach().float().contiguous()
            basis = torch.empty(batch, m + 1, 2 * n * n, device=dev)
            hess = torch.empty(batch, m + 1, m, 2, device=dev)
            x32 = torch.zeros(batch, 2, n, n, device=dev)
            x64 = torch.zeros(batch, 2, n, n, device=dev, dtype=torch.float64)
            run = {"plain": lambda: [eng.gmres_cycle(x32, k_sq, src, m, 0.0, basis, hess) for _ in range(a.cycles)],
                   "refined": lambda: [eng.gmres_refine_cycle(x64, k_sq, src, m, 0.0, 0.0, basis, hess) for _ in range(a.cycles)]}
            for b in run:
                run[b]()                                   # warm: workspaces, float64 tables, kernels
            t = {"plain": [], "refined": []}
            for _ in range(a.rounds):
                for b in ("plain", "refined"):
                    t[b].append(_timed(run[b]) / a.cycles)
            k64, s64 = k_sq.double(), src.double()
            reps = 50
            t_op = min(_timed(lambda: [eng.residual64(x64, k64, s64, True, True) for _ in range(reps)]) / reps for _ in range(3))
            plain, refined = statistics.median(t["plain"]), statistics.median(t["refined"])
            rows.append({"shape": f"{n}x{n} x {batch}", "restart": m, "plain_cycle_s": plain, "refined_cycle_s": refined, "ratio": refined / plain,
                         "plain_spread": [min(t["plain"]), max(t["plain"])], "refined_spread": [min(t["refined"]), max(t["refined"])],
                         "float64_operator_s": t_op, "extra_s": refined - plain})
    props = torch.cuda.get_device_properties(0)
    out = {"device": props.name, "hwmon": hw.summary(), "cycles_per_window": a.cycles, "rounds": a.rounds, "f64_fft": a.f64_fft, "rows": rows}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
