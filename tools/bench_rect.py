"""Time of the spectral residual and of one solver iteration on a rectangular H x W domain (hn_set_domain_rect) next to the same call on the square
the problem has to be padded to without it, both in this process, alternating.

    python tools/bench_rect.py [--regions 7] [--rounds 2] [--cases 256x1024x8:1024,128x512x32:512,208x1040x2:1040] [--out profiles/rect_bench.txt]

Per case H x W x batch : n (the padded square n x n, same batch) two contexts with the shipped weights, one per domain.  5 warm-up calls, then --regions
timed regions (device events on the caller's stream around enough back-to-back calls to fill ~30 ms); the two domains take turns --rounds times and the
figure is the median over all regions of a domain, in ms per call (hn_residual) or per iteration (hn_step, 4 iterations per call, fp32).  Beside it the
median shader clock (the board's hwmon readings while that domain's regions ran).  The square takes whatever route hn_set_domain gives it with the
default options (1040: the dense operator).
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

PML, SIGMA_MAX, K = 8, 2.0, 1.0
DEV = torch.device("cuda:0")
ROUTES = {1: "pow2", 2: "prime_factor", 3: "dense", 4: "mixed", 5: "rectangular"}
ITERS = 4


def region_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(fns, regions, rounds):
    """[(median ms per call, median shader clock in MHz or None)] for the callables in `fns`, which take turns."""
    times, clocks = [[] for _ in fns], [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            reps = max(1, min(500, math.ceil(30.0 / max(region_ms(fn, 2), 1e-3))))
            hw = Hwmon(DEV)
            with hw:
                times[i] += [region_ms(fn, reps) for _ in range(regions)]
            s = hw.summary()
            if s and "sclk_mhz_median" in s:
                clocks[i].append(s["sclk_mhz_median"])
    return [(statistics.median(t), statistics.median(c) if c else None) for t, c in zip(times, clocks)]


def problem(eng, h, w, batch, seed):
    g = torch.Generator().manual_seed(seed)
    k_sq = ((1.0 / (1.0 + torch.rand(batch, 1, h, w, generator=g))) ** 2).to(DEV)
    src = torch.zeros(1, 2, h, w)
    src[0, 0, h // 4, w // 2] = 10.0
    src = src.to(DEV)
    wf = torch.randn(batch, 2, h, w, generator=g).to(DEV)
    state = {"wf": torch.zeros(batch, 2, h, w, device=DEV), "st": torch.zeros(batch, 2, eng.state_len, device=DEV)}
    state["res"] = eng.residual(state["wf"], k_sq, src)
    return (lambda: eng.residual(wf, k_sq, src)), (lambda: eng.step(state["wf"], state["res"], state["st"], k_sq, src, ITERS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cases", default="256x1024x8:1024,128x512x32:512,208x1040x2:1040")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine, pack_weights
    solver = IterativeSolver.from_exported_weights()
    hp = solver.hparams
    blob = pack_weights(dict(solver.f.state_dict()), hp.depth, hp.activation_function, hp.state_depth)
    clk = lambda c: f"{c:6.0f}" if c else "   n/a"  # noqa: E731
    head = "case                          call           rect ms   sclk    square ms   sclk   square/rect   area ratio"
    lines = [f"rectangular domain (hn_set_domain_rect) against the padded square (hn_set_domain) on {torch.cuda.get_device_name(DEV)}",
             f"median of {args.rounds} x {args.regions} timed regions of ~30 ms each; hn_residual: ms per call, hn_step: ms per iteration (fp32, shipped weights); "
             "sclk = median shader clock in MHz while the regions ran", "", head]
    print("\n".join(lines), flush=True)
    for case in args.cases.split(","):
        shape, n = case.split(":")
        h, w, batch = (int(v) for v in shape.split("x"))
        n = int(n)
        engs = []
        for dom in ((h, w), (n, n)):
            e = Engine(DEV)
            e.load_weights(blob, hp.features, hp.depth, hp.state_channels, hp.activation_function)
            e.set_domain_rect(dom[0], dom[1], PML, SIGMA_MAX, K)
            e.reserve(batch)
            engs.append(e)
        routes = [ROUTES.get(e.counter("spectral_route")) for e in engs]
        assert routes[0] == "rectangular", routes
        calls = [problem(engs[0], h, w, batch, 7 * h + w), problem(engs[1], n, n, batch, n)]
        for j, name in enumerate(("hn_residual", "hn_step")):
            (tr, cr), (ts, cs) = measure([calls[0][j], calls[1][j]], args.regions, args.rounds)
            if j == 1:
                tr, ts = tr / ITERS, ts / ITERS
            lines.append(f"{shape + ' : ' + str(n) + '^2 (' + routes[1] + ')':<29} {name:<12} {tr:9.4f} {clk(cr)}   {ts:10.4f} {clk(cs)}   {ts / tr:10.2f}   {n * n / (h * w):10.2f}")
            print(lines[-1], flush=True)
        for e in engs:
            e.check_async_errors()
            e.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
