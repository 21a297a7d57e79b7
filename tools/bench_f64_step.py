"""Time of one solver iteration in float64 (hn_step_f64: the layer-by-layer UNet of hn_unet_f64.hip + the float64 residual on the route --f64-fft
picks: 0 dense, 1 FFT) next to the fp32 hn_step on the same problem.

    python tools/bench_f64_step.py [--iters 20] [--calls 7] [--sizes 96x8,256x4,512x1] [--f64-fft 0] [--out profiles/f64_step.txt]

Per size (n^2 x batch): median over --calls timed calls of --iters iterations each (device events on the caller's stream) after one warm-up call of each
path, the two paths alternating call by call so that both see the same clocks.  Shipped weights, ring phantoms, the solver's point source.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helmnet_amd import IterativeSolver  # noqa: E402
from helmnet_amd.phantoms import ring_sos_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--sizes", default="96x8,256x4,512x1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--f64-fft", type=int, default=0, choices=(0, 1), help="route of the float64 residual (option 'f64_fft')")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    solver = IterativeSolver.from_exported_weights()
    solver.freeze()
    solver.to(dev)
    lines = [f"one solver iteration, median over {args.calls} calls of {args.iters} iterations (ms per iteration): hn_step_f64 (f64_fft {args.f64_fft}) vs hn_step (fp32)",
             "size        hn_step_f64      hn_step   ratio (f64 / fp32)   max|wf32 - wf64|"]
    for size in args.sizes.split(","):
        n, batch = (int(v) for v in size.split("x"))
        solver.set_domain_size(n, source_location=[n - n // 7, n // 2])
        sos = torch.from_numpy(ring_sos_batch(n, batch, seed=n)).to(dev)
        eng = solver.engine()
        eng.set_option("f64_fft", args.f64_fft)
        k32, wf32 = solver.get_initials(sos)
        k32 = k32.contiguous()
        src32, src64 = solver._src(), solver.source.detach().double().contiguous()
        st32 = torch.zeros(batch, 2, eng.state_len, device=dev)
        res32 = eng.residual(wf32, k32, src32)
        wf64, k64, st64 = wf32.double(), ((solver.hparams.omega / sos.double()) ** 2).contiguous(), st32.double()
        res64 = eng.residual64(wf64, k64, src64, True, False)[0]
        paths = {"f64": lambda: eng.step64(wf64, res64, st64, k64, src64, args.iters), "f32": lambda: eng.step(wf32, res32, st32, k32, src32, args.iters)}
        times = {"f64": [], "f32": []}
        for call in range(args.calls + 1):          # call 0 warms up (and builds the float64 buffers)
            for name, fn in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if call == 1:
                    apart = float((wf32.double() - wf64).abs().max())      # after the same number of iterations on both paths
                if call > 0:
                    times[name].append(a.elapsed_time(b) / args.iters)
        t64, t32 = statistics.median(times["f64"]), statistics.median(times["f32"])
        lines.append(f"{n}^2 x {batch:<4} {t64:11.3f} {t32:12.3f} {t64 / t32:20.1f} {apart:18.2e}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
