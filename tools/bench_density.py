"""Cost of a heterogeneous density: hn_residual_medium next to hn_residual_lossy -- the same LDS-line kernel family, so the ratio is the price of the
two rho_grad plane reads -- and next to hn_residual on the domain's own route; and one hn_step_medium iteration next to one hn_step_lossy iteration.
All on the same square domain, in this process, alternating.

    python tools/bench_density.py [--regions 7] [--rounds 2] [--cases 256x32,512x16,400x16] [--tables forward,adjoint] [--out profiles/density_bench.txt]

Per case n x batch one context with the shipped weights.  hn_residual runs on the domain's own spectral route (256, 512: the register-resident kernels;
400 = 25 * 16: the dense operator), the lossy and the variable-density calls on the general LDS-line kernel of hn_spectral_line.hip.  5 warm-up calls,
then --regions timed regions (device events on the caller's stream around enough back-to-back calls to fill ~30 ms); the calls take turns --rounds
times and the figure is the median over all regions, in ms per call (residual) or per iteration (step, 4 iterations per call, fp32).  Beside it the
median shader clock (the board's hwmon readings while that call's regions ran).

The third table (``--tables adjoint``; with it alone the tables already in ``--out`` are kept and this one is replaced) is the adjoint side:
hn_residual_vjp_medium next to hn_residual_vjp_lossy and next to hn_residual_medium, and hn_adjoint_grad_medium (the pointwise launch plus the two
first-derivative passes) next to hn_adjoint_grad_lossy (the pointwise launch alone), measured the same way.

From the traffic alone -- two more fp32 reads per pixel on about 56 bytes (wavefield 8 in each pass, the column pass's 8 out and 8 back in, k_sq 4,
k_sq_im 4, the wavefield's 8 again, the residual 8) -- the variable-density residual should cost at most 1.14 x the lossy one.
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
    """(lossy, variable-density, lossless residual), (lossy step, variable-density step) as callables on one medium; each loop owns its wavefield,
    residual and states."""
    g = torch.Generator().manual_seed(seed)
    sos = 1.0 + torch.rand(batch, 1, n, n, generator=g)
    alpha = 0.1 * torch.rand(batch, 1, n, n, generator=g)
    k = 1.0 / sos
    k_sq, k_im = (k ** 2 - alpha ** 2).to(DEV), (2.0 * k * alpha).to(DEV)
    rho = (0.8 * torch.rand(batch, 2, n, n, generator=g) - 0.4).to(DEV)
    src = torch.zeros(1, 2, n, n)
    src[0, 0, n // 4, n // 2] = 10.0
    src = src.to(DEV)
    wf = torch.randn(batch, 2, n, n, generator=g).to(DEV)

    def loop(medium):
        st = {"wf": torch.zeros(batch, 2, n, n, device=DEV), "st": torch.zeros(batch, 2, eng.state_len, device=DEV)}
        if medium:
            st["res"] = eng.residual_medium(st["wf"], k_sq, k_im, rho, src)
            return lambda: eng.step_medium(st["wf"], st["res"], st["st"], k_sq, k_im, rho, src, ITERS)
        st["res"] = eng.residual_lossy(st["wf"], k_sq, k_im, src)
        return lambda: eng.step_lossy(st["wf"], st["res"], st["st"], k_sq, k_im, src, ITERS)

    residuals = ((lambda: eng.residual_lossy(wf, k_sq, k_im, src)), (lambda: eng.residual_medium(wf, k_sq, k_im, rho, src)),
                 (lambda: eng.residual(wf, k_sq, src)))
    return residuals, (loop(False), loop(True))


ADJOINT_MARK = "the adjoint side (hn_residual_vjp_medium, hn_adjoint_grad_medium)"


def adjoint_problem(eng, n, batch, seed):
    """(lossy adjoint, variable-density adjoint, variable-density forward), (lossy gradient call, variable-density gradient call) on one medium."""
    g = torch.Generator().manual_seed(seed)
    sos = 1.0 + torch.rand(batch, 1, n, n, generator=g)
    alpha = 0.1 * torch.rand(batch, 1, n, n, generator=g)
    k = 1.0 / sos
    k_sq, k_im = (k ** 2 - alpha ** 2).to(DEV), (2.0 * k * alpha).to(DEV)
    rho = (0.8 * torch.rand(batch, 2, n, n, generator=g) - 0.4).to(DEV)
    src = torch.zeros(1, 2, n, n, device=DEV)
    cot, lam, u = (torch.randn(batch, 2, n, n, generator=g).to(DEV) for _ in range(3))
    operators = ((lambda: eng.residual_vjp_lossy(cot, k_sq, k_im)), (lambda: eng.residual_vjp_medium(cot, k_sq, k_im, rho)),
                 (lambda: eng.residual_medium(cot, k_sq, k_im, rho, src)))
    grads = ((lambda: eng.adjoint_grad_lossy(lam, u, None)), (lambda: eng.adjoint_grad_medium(lam, u, None)))
    return operators, grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--cases", default="256x32,512x16,400x16")
    ap.add_argument("--tables", default="forward,adjoint")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "density_bench.txt"))
    args = ap.parse_args()
    tables = args.tables.split(",")
    from helmnet_amd import IterativeSolver
    from helmnet_amd.engine import Engine, pack_weights
    solver = IterativeSolver.from_exported_weights()
    hp = solver.hparams
    blob = pack_weights(dict(solver.f.state_dict()), hp.depth, hp.activation_function, hp.state_depth)
    clk = lambda c: f"{c:6.0f}" if c else "   n/a"  # noqa: E731
    lines = [f"heterogeneous density (hn_residual_medium, hn_step_medium) against the lossy and the lossless calls on {torch.cuda.get_device_name(DEV)}",
             f"median of {args.rounds} x {args.regions} timed regions of ~30 ms each, the calls taking turns in one process; residual: ms per call, step: ms "
             "per iteration (fp32, shipped weights); sclk = median shader clock in MHz while the regions ran", "",
             "case                      call             lossy ms   sclk    medium ms   sclk   medium/lossy   lossless ms   sclk   medium/lossless"]
    if "forward" not in tables:      # keep what the file has of the first two tables
        lines = []
        if args.out and os.path.exists(args.out):
            lines = open(args.out).read().split("\n")
            lines = lines[:lines.index(ADJOINT_MARK)] if ADJOINT_MARK in lines else lines
            while lines and not lines[-1]:
                lines.pop()
    print("\n".join(lines), flush=True)
    for case in args.cases.split(",") if "forward" in tables else ():
        n, batch = (int(v) for v in case.split("x"))
        e = Engine(DEV)
        e.load_weights(blob, hp.features, hp.depth, hp.state_channels, hp.activation_function)
        e.set_domain(n, PML, SIGMA_MAX, K)
        e.reserve(batch)
        route = ROUTES.get(e.counter("spectral_route"))
        tag = f"{str(n) + '^2 x ' + str(batch) + ' (' + str(route) + ')':<25}"
        residuals, steps = problem(e, n, batch, 13 * n + batch)
        (tl, cl), (tm, cm), (t0, c0) = measure(list(residuals), args.regions, args.rounds)
        lines.append(f"{tag} {'residual':<12} {tl:12.4f} {clk(cl)}   {tm:10.4f} {clk(cm)}   {tm / tl:12.3f}   {t0:11.4f} {clk(c0)}   {tm / t0:15.2f}")
        print(lines[-1], flush=True)
        (tl, cl), (tm, cm) = measure(list(steps), args.regions, args.rounds)
        tl, tm = tl / ITERS, tm / ITERS
        lines.append(f"{tag} {'step':<12} {tl:12.4f} {clk(cl)}   {tm:10.4f} {clk(cm)}   {tm / tl:12.3f}")
        print(lines[-1], flush=True)
        e.check_async_errors()
        e.close()
    if "adjoint" in tables:
        lines += ["", ADJOINT_MARK, "same method; operator and gradient call: ms per call; vjp = hn_residual_vjp_*, grad = hn_adjoint_grad_* (lossy: one "
                  "pointwise launch; medium: that launch and the two first-derivative passes)", "",
                  "case                      call             lossy ms   sclk    medium ms   sclk   medium/lossy   forward medium ms   sclk   adjoint/forward"]
        print("\n".join(lines[-5:]), flush=True)
        for case in args.cases.split(","):
            n, batch = (int(v) for v in case.split("x"))
            e = Engine(DEV)
            e.set_domain(n, PML, SIGMA_MAX, K)
            route = ROUTES.get(e.counter("spectral_route"))
            tag = f"{str(n) + '^2 x ' + str(batch) + ' (' + str(route) + ')':<25}"
            operators, grads = adjoint_problem(e, n, batch, 17 * n + batch)
            (tl, cl), (tm, cm), (tf, cf) = measure(list(operators), args.regions, args.rounds)
            lines.append(f"{tag} {'vjp':<12} {tl:12.4f} {clk(cl)}   {tm:10.4f} {clk(cm)}   {tm / tl:12.3f}   {tf:17.4f} {clk(cf)}   {tm / tf:15.3f}")
            print(lines[-1], flush=True)
            (tl, cl), (tm, cm) = measure(list(grads), args.regions, args.rounds)
            lines.append(f"{tag} {'grad':<12} {tl:12.4f} {clk(cl)}   {tm:10.4f} {clk(cm)}   {tm / tl:12.3f}")
            print(lines[-1], flush=True)
            e.check_async_errors()
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
