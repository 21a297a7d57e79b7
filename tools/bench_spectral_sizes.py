"""Time of the spectral residual at domain sizes n = P * 2^k with an odd P >= 9: the dense n x n operator (spectral_mixed 0: k_spec_dense) next
to the mixed FFT kernels (spectral_mixed 1: k_spec_line, hn_spectral_line.hip), both in this process on the same inputs.

    python tools/bench_spectral_sizes.py [--regions 7] [--rounds 2] [--sizes 144x32,...] [--step-sizes 400x16,1040x2] [--out profiles/spectral_mixed_bench.txt]

Per size (n^2 x batch) and option value: 5 warm-up calls, then --regions timed regions (device events on the caller's stream around enough
back-to-back hn_residual calls to fill ~30 ms); the two values take turns --rounds times and the figure is the median over all regions of a value, in
ms per call.  Beside it the median shader clock (the board's hwmon readings while that value's regions ran) and the largest difference of the two
results as a fraction of max|residual|.  At --step-sizes the same for one whole solver iteration (hn_step with the shipped weights, ms per iteration).
"""
import argparse
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench import Hwmon  # noqa: E402
from helmnet_amd.laplacian import spectral_route  # noqa: E402

PML, SIGMA_MAX, K = 8, 2.0, 1.0
DEV = torch.device("cuda:0")
ROUTES = {3: "dense", 4: "mixed"}


def region_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(eng, fn, regions, rounds):
    """{option value: (median ms per call, median shader clock in MHz or None)}; `fn` runs one call on the engine's current route."""
    times, clocks = {0: [], 1: []}, {0: [], 1: []}
    for _ in range(rounds):
        for value in (0, 1):
            eng.set_option("spectral_mixed", value)
            assert ROUTES.get(eng.counter("spectral_route")) == ("mixed" if value else "dense"), eng.counter("spectral_route")
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            reps = max(1, min(500, math.ceil(30.0 / max(region_ms(fn, 2), 1e-3))))
            hw = Hwmon(DEV)
            with hw:
                times[value] += [region_ms(fn, reps) for _ in range(regions)]
            s = hw.summary()
            if s and "sclk_mhz_median" in s:
                clocks[value].append(s["sclk_mhz_median"])
    return {v: (statistics.median(times[v]), statistics.median(clocks[v]) if clocks[v] else None) for v in (0, 1)}


def row(label, r, diff):
    clk = lambda c: f"{c:6.0f}" if c else "   n/a"
    (t0, c0), (t1, c1) = r[0], r[1]
    return f"{label:<22} {t0:10.4f} {clk(c0)}   {t1:10.4f} {clk(c1)}   {t0 / t1:8.2f}   {diff:10.2e}"


def parse(sizes):
    return [tuple(int(v) for v in s.split("x")) for s in sizes.split(",") if s]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", default="144x32,240x32,400x16,576x8,1040x2,1152x2,2032x1")
    ap.add_argument("--step-sizes", default="400x16,1040x2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine
    head = "size                     dense ms   sclk     mixed ms   sclk   dense/mixed   max|diff|/max"
    lines = [f"spectral residual, dense operator (spectral_mixed 0) against the mixed FFT kernels (spectral_mixed 1) on {torch.cuda.get_device_name(DEV)}",
             f"median of {args.rounds} x {args.regions} timed regions of ~30 ms each, ms per call; sclk = median shader clock in MHz while the regions ran",
             "", "hn_residual", head]
    print("\n".join(lines), flush=True)
    eng = Engine(DEV)
    for n, batch in parse(args.sizes):
        name, p, q = spectral_route(n, mixed=1)
        if name != "mixed":
            raise SystemExit(f"{n} is not a size of the mixed route ({name})")
        eng.set_option("spectral_mixed", 0)
        eng.set_domain(n, PML, SIGMA_MAX, K)
        g = torch.Generator().manual_seed(n)
        wf = torch.randn(batch, 2, n, n, generator=g).to(DEV)
        k_sq = ((1.0 / (1.0 + torch.rand(batch, 1, n, n, generator=g))) ** 2).to(DEV)
        src = torch.randn(1, 2, n, n, generator=g).to(DEV)
        dense = eng.residual(wf, k_sq, src)
        r = measure(eng, lambda: eng.residual(wf, k_sq, src), args.regions, args.rounds)
        diff = float((eng.residual(wf, k_sq, src) - dense).abs().max() / dense.abs().max())      # the engine is on the mixed route now
        lines.append(row(f"{n}^2 x {batch} ({p} x {q})", r, diff))
        print(lines[-1], flush=True)
    eng.close()
    lines += ["", "one solver iteration (hn_step, shipped weights, fp32)", head]
    print("\n".join(lines[-3:]), flush=True)
    solver = IterativeSolver.from_exported_weights()
    solver.freeze()
    solver.to(DEV)
    for n, batch in parse(args.step_sizes):
        _, p, q = spectral_route(n, mixed=1)
        solver.set_domain_size(n, source_location=[n // 8 + 4, n // 2])
        eng = solver.engine()
        g = torch.Generator().manual_seed(n)
        k_sq = ((1.0 / (1.0 + torch.rand(batch, 1, n, n, generator=g))) ** 2).to(DEV)
        src = solver._src()
        iters = 4

        def fresh():
            wf = torch.zeros(batch, 2, n, n, device=DEV)
            return wf, eng.residual(wf, k_sq, src), torch.zeros(batch, 2, eng.state_len, device=DEV)

        state = {}

        def step():
            eng.step(state["wf"], state["res"], state["st"], k_sq, src, iters)

        ends = {}
        try:
            for value in (0, 1):                                   # the wavefield after `iters` iterations from zero, per route
                eng.set_option("spectral_mixed", value)
                state["wf"], state["res"], state["st"] = fresh()
                step()
                ends[value] = state["wf"].clone()
            state["wf"], state["res"], state["st"] = fresh()
            r = measure(eng, step, args.regions, args.rounds)
        finally:
            eng.set_option("spectral_mixed", 0)
        r = {v: (t / iters, c) for v, (t, c) in r.items()}
        diff = float((ends[1] - ends[0]).abs().max() / ends[0].abs().max())
        lines.append(row(f"{n}^2 x {batch} ({p} x {q})", r, diff))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
