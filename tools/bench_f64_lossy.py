"""Time of the float64 lossy residual (hn_residual_f64_lossy) and of one lossy refinement cycle (hn_fgmres_refine_cycle_lossy) next to their
lossless siblings on the same route.

    python tools/bench_f64_lossy.py [--calls 30] [--out profiles/f64_lossy_bench.txt]

Three measurements in one process, the two paths of each alternating call by call after 5 warm-up calls of each, device events on the caller's stream,
the median of --calls calls:
    1  hn_residual_f64_lossy next to hn_residual_f64 on the FFT route (option 'f64_fft' 1) at 256^2 x 32, 512^2 x 16 and 2048^2 x 1 (res + rmse);
    2  hn_residual_f64_lossy on a 256 x 1024 x 8 rectangle (the lossless entry point has no rectangular form);
    3  one hn_fgmres_refine_cycle_lossy next to one hn_fgmres_refine_cycle, restart 20 and no preconditioner iterations, at 256^2 x 8, from x = 0.
Needs a GPU: without one it fails.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helmnet_amd.engine import Engine  # noqa: E402

PML, SIGMA_MAX, K = 8, 2.0, 1.0


def timed(paths, calls):
    """Median ms of each path, the paths alternating call by call after 5 warm-up calls of each."""
    for _ in range(5):
        for _, fn in paths:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in paths}
    for _ in range(calls):
        for name, fn in paths:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    return {name: statistics.median(v) for name, v in times.items()}


def fields(h, w, batch, dev, dtype):
    g = torch.Generator().manual_seed(h + w)
    wf = torch.randn(batch, 2, h, w, generator=g, dtype=dtype).to(dev)
    k_sq = ((1.0 / (1.0 + torch.rand(batch, 1, h, w, generator=g, dtype=dtype))) ** 2).to(dev)
    k_im = (0.2 * torch.rand(batch, 1, h, w, generator=g, dtype=dtype)).to(dev)
    src = torch.randn(1, 2, h, w, generator=g, dtype=dtype).to(dev)
    return wf, k_sq, k_im, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default="profiles/f64_lossy_bench.txt")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f64_lossy.py needs a GPU")
    dev = torch.device("cuda:0")
    eng = Engine(dev)
    lines = [f"float64 lossy residual and refinement cycle on {torch.cuda.get_device_properties(dev).name}, median of {args.calls} calls (ms), "
             "the two paths of a row alternating in one process",
             "1  hn_residual_f64_lossy next to hn_residual_f64 on the FFT route (res + rmse)",
             "size             lossless     lossy   lossy / lossless"]
    for n, batch in ((256, 32), (512, 16), (2048, 1)):
        eng.set_domain(n, PML, SIGMA_MAX, K)
        eng.set_option("f64_fft", 1)
        wf, k_sq, k_im, src = fields(n, n, batch, dev, torch.float64)
        t = timed((("lossless", lambda: eng.residual64(wf, k_sq, src)), ("lossy", lambda: eng.residual64_lossy(wf, k_sq, k_im, src))), args.calls)
        assert eng.counter("f64_route") == 2
        lines.append(f"{n}^2 x {batch:<6} {t['lossless']:10.3f} {t['lossy']:9.3f} {t['lossy'] / t['lossless']:18.3f}")
        print(lines[-1], flush=True)
        del wf, k_sq, k_im, src
    eng.set_option("f64_fft", 0)
    h, w, batch = 256, 1024, 8
    eng.set_domain_rect(h, w, PML, SIGMA_MAX, K)
    wf, k_sq, k_im, src = fields(h, w, batch, dev, torch.float64)
    t = timed((("lossy", lambda: eng.residual64_lossy(wf, k_sq, k_im, src)),), args.calls)
    lines += ["2  hn_residual_f64_lossy on a rectangle (res + rmse)", f"{h} x {w} x {batch}: {t['lossy']:.3f}"]
    print(lines[-1], flush=True)
    del wf, k_sq, k_im, src
    n, batch, restart = 256, 8, 20
    eng.set_domain(n, PML, SIGMA_MAX, K)
    eng.set_option("f64_fft", 1)          # the lossless cycle's float64 residual on the route the lossy one always takes
    _, k_sq, k_im, rhs = fields(n, n, batch, dev, torch.float32)
    x = torch.zeros(batch, 2, n, n, device=dev, dtype=torch.float64)
    basis = torch.empty(batch, restart + 1, 2 * n * n, device=dev)
    zbasis = torch.empty(batch, restart, 2 * n * n, device=dev)
    hess = torch.empty(batch, restart + 1, restart, 2, device=dev)

    def cycle(lossy):
        def call():
            x.zero_()
            if lossy:
                eng.fgmres_refine_cycle_lossy(x, k_sq, k_im, rhs, restart, 1e-10, 0, 1.0, 1e-6, basis, hess, zbasis)
            else:
                eng.fgmres_refine_cycle(x, k_sq, rhs, restart, 1e-10, 0, 1.0, 1e-6, basis, hess, zbasis)
        return call

    t = timed((("lossless", cycle(False)), ("lossy", cycle(True))), args.calls)
    eng.check_async_errors()
    lines += [f"3  one refinement cycle, restart {restart}, no preconditioner iterations, from x = 0 (hn_fgmres_refine_cycle_lossy next to hn_fgmres_refine_cycle)",
              "size             lossless     lossy   lossy / lossless",
              f"{n}^2 x {batch:<6} {t['lossless']:10.3f} {t['lossy']:9.3f} {t['lossy'] / t['lossless']:18.3f}"]
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
