"""Time of the float64 residual (hn_residual_f64) on its two routes -- option 'f64_fft' 0: dense circulant operators on the f64 matrix instruction, 1: two
FFT line passes in double (hn_f64_fft.hip) -- next to the reference's own way of getting the same answer on the same GPU: its formulation in torch.fft on
complex128 tensors (spectral.py:31-79 + hybridnet.py:544-556 under .double()).

    python tools/bench_f64_residual.py [--calls 50] [--sizes 256x32,512x16,1024x4,2048x1] [--out profiles/f64_fft_bench.txt]

Per size (n^2 x batch): median of --calls timed calls (device events on the caller's stream) after 5 warm-up calls of each path, the three paths
alternating call by call in one process so that all see the same clocks (the option is flipped between calls; each route keeps its tables); the
agreement of each route with torch.fft is printed beside the times, and the median shader clock of the board's hwmon readings while the size ran.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import Hwmon  # noqa: E402
from helmnet_amd.engine import Engine  # noqa: E402

PML, SIGMA_MAX, K = 8, 2.0, 1.0


def torch_tables(n, dev):
    """The reference's buffers after .double(): fp32 values carried in complex128 (k grid with Nyquist at -pi, fp32 square, fp32-rounded PML coefficients)."""
    k = 2.0 * np.pi * np.linspace(-0.5, 0.5, n, endpoint=False)
    k1 = np.concatenate((k[n // 2:], k[: n // 2])).astype(np.float32)
    k2 = -(k1 * k1)
    coord = np.arange(PML)
    sigma, sigp = np.zeros(n), np.zeros(n)
    so, sp = SIGMA_MAX * np.abs(1 - coord / PML) ** 2, -2 * SIGMA_MAX * (1 - coord / PML) / PML
    sigma[:PML], sigma[-PML:] = so, so[::-1]
    sigp[:PML], sigp[-PML:] = sp, -sp[::-1]
    inv_gamma = 1.0 / (1.0 + (1j / K) * sigma)
    a, b = -(1j / K) * sigp * inv_gamma ** 3, inv_gamma ** 2

    def c32(z):
        return torch.from_numpy(z.real.astype(np.float32).astype(np.float64) + 1j * z.imag.astype(np.float32).astype(np.float64)).to(dev)

    return (torch.from_numpy(1j * k1.astype(np.float64)).to(dev), torch.from_numpy(k2.astype(np.float64) + 0j).to(dev), c32(a), c32(b))


def torch_residual(u, k_sq, src, tab):
    ik, k2, a, b = tab
    uf = torch.fft.fftn(u, dim=(-2, -1))
    d = torch.fft.ifftn(torch.stack([uf * ik, uf * ik[:, None], uf * k2, uf * k2[:, None]]), dim=(-2, -1))
    return a * d[0] + a[:, None] * d[1] + b * d[2] + b[:, None] * d[3] + k_sq * u - src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--sizes", default="256x32,512x16,1024x4,2048x1")
    ap.add_argument("--out", default="profiles/f64_fft_bench.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = Engine(dev)
    lines = [f"float64 residual (res + rmse) on {torch.cuda.get_device_properties(dev).name}, median of {args.calls} calls (ms), the three paths alternating in one process:",
             "hn_residual_f64 dense (f64_fft 0), hn_residual_f64 FFT (f64_fft 1), torch.fft on complex128; max|diff| / max|res| of each route against torch.fft",
             "size            dense       fft   torch.fft   fft / dense   fft / torch   diff dense    diff fft   sclk MHz"]
    for size in args.sizes.split(","):
        n, batch = (int(v) for v in size.split("x"))
        eng.set_domain(n, PML, SIGMA_MAX, K)
        g = torch.Generator().manual_seed(n)
        wf = torch.randn(batch, 2, n, n, generator=g, dtype=torch.float64).to(dev)
        k_sq = ((1.0 / (1.0 + torch.rand(batch, 1, n, n, generator=g, dtype=torch.float64))) ** 2).to(dev)
        src = torch.randn(1, 2, n, n, generator=g, dtype=torch.float64).to(dev)
        tab = torch_tables(n, dev)
        u_c, src_c, k_c = torch.complex(wf[:, 0], wf[:, 1]), torch.complex(src[:, 0], src[:, 1]), k_sq[:, 0]

        def route(fft):
            def call():
                eng.set_option("f64_fft", fft)
                return eng.residual64(wf, k_sq, src)
            return call

        def ref():
            r = torch_residual(u_c, k_c, src_c, tab)
            return r, torch.view_as_real(r).pow(2).mean((1, 2, 3)).sqrt()

        paths = (("dense", route(0)), ("fft", route(1)), ("ref", ref))
        for _ in range(5):
            got = {name: fn() for name, fn in paths}
        torch.cuda.synchronize()
        assert eng.counter("f64_route") == 2
        want = got["ref"][0]
        diff = {name: float(max((got[name][0][:, 0] - want.real).abs().max(), (got[name][0][:, 1] - want.imag).abs().max()) / want.abs().max())
                for name in ("dense", "fft")}
        del got, want
        times = {name: [] for name, _ in paths}
        hw = Hwmon(dev)
        with hw:
            for _ in range(args.calls):
                for name, fn in paths:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times[name].append(a.elapsed_time(b))
        clock = (hw.summary() or {}).get("sclk_mhz_median")
        t = {name: statistics.median(v) for name, v in times.items()}
        lines.append(f"{n}^2 x {batch:<4} {t['dense']:10.3f} {t['fft']:9.3f} {t['ref']:11.3f} {t['fft'] / t['dense']:13.2f} {t['fft'] / t['ref']:13.2f} "
                     f"{diff['dense']:12.2e} {diff['fft']:11.2e}   {clock if clock is not None else 'n/a'}")
        print(lines[-1], flush=True)
    eng.set_option("f64_fft", 0)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
