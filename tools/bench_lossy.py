"""Cost of an absorbing medium: hn_residual_lossy next to hn_residual and one hn_step_lossy iteration next to one hn_step iteration, on the same
square domain, in this process, alternating; and (--parts adjoint) the lossy adjoint hn_residual_vjp_lossy next to hn_residual_lossy, which does the
same transform work, and next to the lossless hn_residual_vjp on the domain's own route, the lower bound.

    python tools/bench_lossy.py [--regions 7] [--rounds 2] [--cases 256x32,512x16,400x16] [--parts forward,adjoint] [--append]
                                [--out profiles/lossy_bench.txt]

Per case n x batch one context with the shipped weights.  The lossless calls run on the domain's own spectral route (256, 512: the register-resident
kernels; 400 = 25 * 16: the dense operator), the lossy ones on the general LDS-line kernel of hn_spectral_line.hip with the complex pointwise term.
5 warm-up calls, then --regions timed regions (device events on the caller's stream around enough back-to-back calls to fill ~30 ms); the two calls
take turns --rounds times and the figure is the median over all regions, in ms per call (residual) or per iteration (step, 4 iterations per call,
fp32).  Beside it the median shader clock (the board's hwmon readings while that call's regions ran).
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_rect import DEV, ITERS, K, PML, ROUTES, SIGMA_MAX, measure  # noqa: E402


def problem(eng, n, batch, seed):
    """(lossless residual, lossy residual), (lossless step, lossy step) as callables on one medium; each loop owns its wavefield, residual and states."""
    g = torch.Generator().manual_seed(seed)
    sos = 1.0 + torch.rand(batch, 1, n, n, generator=g)
    alpha = 0.1 * torch.rand(batch, 1, n, n, generator=g)
    k = 1.0 / sos
    k_sq, k_im = (k ** 2 - alpha ** 2).to(DEV), (2.0 * k * alpha).to(DEV)
    src = torch.zeros(1, 2, n, n)
    src[0, 0, n // 4, n // 2] = 10.0
    src = src.to(DEV)
    wf = torch.randn(batch, 2, n, n, generator=g).to(DEV)

    def loop(lossy):
        st = {"wf": torch.zeros(batch, 2, n, n, device=DEV), "st": torch.zeros(batch, 2, eng.state_len, device=DEV)}
        if lossy:
            st["res"] = eng.residual_lossy(st["wf"], k_sq, k_im, src)
            return lambda: eng.step_lossy(st["wf"], st["res"], st["st"], k_sq, k_im, src, ITERS)
        st["res"] = eng.residual(st["wf"], k_sq, src)
        return lambda: eng.step(st["wf"], st["res"], st["st"], k_sq, src, ITERS)

    adjoint = ((lambda: eng.residual_lossy(wf, k_sq, k_im, src)), (lambda: eng.residual_vjp_lossy(wf, k_sq, k_im)), (lambda: eng.residual_vjp(wf, k_sq)))
    return ((lambda: eng.residual(wf, k_sq, src)), (lambda: eng.residual_lossy(wf, k_sq, k_im, src))), (loop(False), loop(True)), adjoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cases", default="256x32,512x16,400x16")
    ap.add_argument("--parts", default="forward,adjoint", help="forward: the lossy calls against the lossless ones; adjoint: hn_residual_vjp_lossy")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lossy_bench.txt"))
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine, pack_weights
    solver = IterativeSolver.from_exported_weights()
    hp = solver.hparams
    blob = pack_weights(dict(solver.f.state_dict()), hp.depth, hp.activation_function, hp.state_depth)
    clk = lambda c: f"{c:6.0f}" if c else "   n/a"  # noqa: E731
    head = "case                      call           lossless ms   sclk     lossy ms   sclk   lossy/lossless"
    lines = [f"absorbing media (hn_residual_lossy, hn_step_lossy) against the lossless calls on {torch.cuda.get_device_name(DEV)}",
             f"median of {args.rounds} x {args.regions} timed regions of ~30 ms each; residual: ms per call, step: ms per iteration (fp32, shipped weights); "
             "sclk = median shader clock in MHz while the regions ran", "", head]
    if "forward" not in parts:
        lines = []
    print("\n".join(lines), flush=True)
    adj_lines = [f"the lossy adjoint (hn_residual_vjp_lossy) against hn_residual_lossy and the lossless hn_residual_vjp on {torch.cuda.get_device_name(DEV)}",
                 f"median of {args.rounds} x {args.regions} timed regions of ~30 ms each, the three calls taking turns in one process; ms per call; sclk = "
                 "median shader clock in MHz while the regions ran", "",
                 "case                      lossy fwd ms   sclk   lossy adj ms   sclk   adj/fwd   lossless adj ms   sclk   lossy adj/lossless adj"]
    for case in args.cases.split(","):
        n, batch = (int(v) for v in case.split("x"))
        e = Engine(DEV)
        e.load_weights(blob, hp.features, hp.depth, hp.state_channels, hp.activation_function)
        e.set_domain(n, PML, SIGMA_MAX, K)
        e.reserve(batch)
        route = ROUTES.get(e.counter("spectral_route"))
        calls = problem(e, n, batch, 11 * n + batch)
        for j, name in enumerate(("residual", "step") if "forward" in parts else ()):
            (t0, c0), (t1, c1) = measure(list(calls[j]), args.regions, args.rounds)
            if j == 1:
                t0, t1 = t0 / ITERS, t1 / ITERS
            lines.append(f"{str(n) + '^2 x ' + str(batch) + ' (' + str(route) + ')':<25} {name:<12} {t0:13.4f} {clk(c0)}   {t1:10.4f} {clk(c1)}   {t1 / t0:14.2f}")
            print(lines[-1], flush=True)
        if "adjoint" in parts:
            (tf, cf), (ta, ca), (tl, cl) = measure(list(calls[2]), args.regions, args.rounds)
            adj_lines.append(f"{str(n) + '^2 x ' + str(batch) + ' (' + str(route) + ')':<25} {tf:12.4f} {clk(cf)}   {ta:12.4f} {clk(ca)}   {ta / tf:7.2f}   "
                             f"{tl:15.4f} {clk(cl)}   {ta / tl:22.2f}")
            print(adj_lines[-1], flush=True)
        e.check_async_errors()
        e.close()
    if "adjoint" in parts:
        lines += ([""] if lines else []) + adj_lines
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(("\n" if args.append else "") + text)


if __name__ == "__main__":
    main()
