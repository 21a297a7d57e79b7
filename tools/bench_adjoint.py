#!/usr/bin/env python
"""What the adjoint-state gradient of a converged solve costs, next to back-propagation through the learned iterations.

    python tools/bench_adjoint.py [--out profiles/adjoint_bench.txt] [--absorption A0] [--density]

At 96^2 x 4 (source [82, 48]) and 256^2 x 4 (source [194, 128]), ring phantoms, the loss J = c/2 sum |u[row 20]|^2 with the constant c chosen so that
the cotangent dJ/du has the source's 2-norm (the adjoint system then asks of the solver what the forward one does), everything to 1e-4:

  implicit     ``solve_implicit(sos, tol)`` + ``backward()`` -- seconds and peak device memory, with the learned preconditioner and without;
  adjoint      the adjoint solve alone (``adjoint_solve`` on the same cotangent): seconds, cycles and UNet evaluations, learned against plain;
  unrolled     ``forward(num_iterations=K, checkpoint_every=25)`` + ``backward()``, K the first iteration count at which the learned solver's worst
               residual RMSE is below the implicit solve's worst final true RMSE -- both then end at the same residual (``K: null`` when
               ``--learned-iterations`` iterations never get there; the row is then measured at that count and says which RMSE it reached).

Time: device events around the whole call on the current stream, the drivers' host reads included; one warm-up, then the median of ``--repeats``
runs.  Peak memory: ``torch.cuda.max_memory_allocated`` over the timed call minus what was allocated before it (the library's own workspaces are
allocated by the warm-up and are not torch's; they are reported as the growth of the device's used memory over the first call).  The shader clock is
the median of the board's hwmon readings while the tool runs (bench.py's sampler), null where the board does not expose it.

``--absorption A0``: the medium absorbs, alpha = A0 nepers per grid point inside the ring (sos > 1.05) and a quarter of it elsewhere.  The implicit and
the adjoint rows then run on the lossy operator and its adjoint; the unrolled row is left out (the solver loop has no gradients with absorption).

``--density``: the medium has the density rho = 1 + 2 (sos - 1), four periodic [1 2 1] / 4 smoothing passes along each axis (bone about twice as
dense as tissue; alone or with ``--absorption``).  The rows run on the variable-density operator and its adjoint, the unrolled row is left out, and the
adjoint solve alone gets a third variant beside learned and plain: ``learned, W alone`` -- the learned preconditioner between the constant-density
similarity weight W (a plane of ones in rho's place) instead of W / rho."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _measure(fn, repeats):
    """(last result, median seconds, [min, max] seconds, peak torch bytes above the starting level, device bytes the first call added)."""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    fn()                                                                  # warm: workspaces, tables, the stream probe
    torch.cuda.synchronize()
    lib_bytes = max(0, free0 - torch.cuda.mem_get_info()[0])
    times, peak, out = [], 0, None
    for _ in range(repeats):
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return out, statistics.median(times), [min(times), max(times)], peak, lib_bytes


def w_alone(s, sos, medium, cot, a):
    """``adjoint_solve(cot, sos, precondition="learned", **medium)`` with ONE difference: the cycle (Engine.fgmres_adjoint_cycle_medium) gets a plane of
    ones where ``gmres_adjoint`` passes rho, so the learned iteration runs between W and not W / rho.  The operator, the host loop
    (``gmres.drive_cycles``), the true-residual check and the keys of the result are ``gmres_adjoint``'s."""
    import numpy as np
    from helmnet_amd.absorption import complex_k_sq
    from helmnet_amd.density import log_density_gradient
    from helmnet_amd.gmres import default_precond_scale, drive_cycles, unet_evaluations
    eng, restart, iters = s.engine(), a.restart, 10
    if "absorption" in medium:
        k_sq, k_im = complex_k_sq(sos.float().contiguous(), medium["absorption"], s.hparams.omega)
    else:
        k_sq, k_im = s.get_initials(sos.float().contiguous())[0].contiguous(), None
    q = log_density_gradient(medium["density"].float().expand_as(k_sq).contiguous())
    ones = torch.ones_like(k_sq)
    alpha = default_precond_scale(s.source)
    bsz, n = sos.shape[0], sos.shape[-1]
    x = torch.zeros(bsz, 2, n, n, device=sos.device)
    basis = torch.empty(bsz, restart + 1, 2 * n * n, device=sos.device)
    zbasis = torch.empty(bsz, restart, 2 * n * n, device=sos.device)
    hess = torch.empty(bsz, restart + 1, restart, 2, device=sos.device)

    def cycle():
        rmse, k_used = eng.fgmres_adjoint_cycle_medium(x, k_sq, k_im, q, ones, cot, restart, a.tol, iters, alpha, basis, zbasis, hess)
        both = torch.cat([rmse.reshape(-1), k_used.float()]).cpu().numpy()
        eng.check_async_errors()
        return both[: (restart + 1) * bsz].reshape(restart + 1, bsz), both[(restart + 1) * bsz:].astype(np.int64)

    def true_residual():
        return eng.rmse(cot - eng.residual_vjp_medium(x, k_sq, k_im, q))

    out = drive_cycles(cycle, lambda: true_residual().cpu().numpy(), a.max_cycles, a.tol)
    final = torch.from_numpy(out["history"][-1]) if out["converged"] else true_residual().cpu()
    return {"cycles": out["cycles"], "iterations": out["iterations"], "converged": out["converged"], "residual_norm": final,
            "operator_applications": out["cycles"] * (restart + 1) + out["true_checks"] + (0 if out["converged"] else 1),
            "unet_evaluations": unet_evaluations(out["cycles"], restart, iters)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="96,256")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-cycles", type=int, default=1500)
    ap.add_argument("--learned-iterations", type=int, default=1000)
    ap.add_argument("--absorption", type=float, default=None, metavar="A0")
    ap.add_argument("--density", action="store_true")
    a = ap.parse_args()
    from bench import Hwmon
    from helmnet_amd import IterativeSolver
    from helmnet_amd.phantoms import ring_sos_batch
    dev, row = "cuda:0", 20
    hw = Hwmon(torch.device(dev))
    rows = []
    with hw:
        for n in [int(t) for t in a.sizes.split(",") if t]:
            s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(dev)
            s.set_domain_size(n, source_location=[82, 48] if n == 96 else [n - 62, n // 2])
            sos = torch.from_numpy(ring_sos_batch(n, a.batch, seed=11)).to(dev)
            src_norm = float(torch.linalg.vector_norm(s.source.detach().double()))
            lossy = {}
            if a.absorption is not None:
                lossy = {"absorption": torch.where(sos > 1.05, torch.full_like(sos, a.absorption), torch.full_like(sos, 0.25 * a.absorption))}
            if a.density:
                rho = 1.0 + 2.0 * (sos - 1.0)
                for _ in range(4):
                    for dim in (-1, -2):
                        rho = 0.25 * torch.roll(rho, 1, dim) + 0.5 * rho + 0.25 * torch.roll(rho, -1, dim)
                lossy["density"] = rho.contiguous()
            u0 = s.gmres(sos, restart=a.restart, max_cycles=a.max_cycles, tol=a.tol, precondition="learned", **lossy)["wavefield"]
            c = src_norm / float(torch.linalg.vector_norm(u0[:, :, row, :].double()) / a.batch ** 0.5)

            def loss(u):
                return 0.5 * c * (u[:, :, row, :] ** 2).sum()

            cot = torch.zeros_like(u0)
            cot[:, :, row, :] = c * u0[:, :, row, :]
            cot = cot.contiguous()

            def implicit(precondition):
                x = sos.clone().requires_grad_(True)
                out = s.solve_implicit(x, tol=a.tol, restart=a.restart, max_cycles=a.max_cycles, precondition=precondition, **lossy)
                loss(out["wavefield"]).backward()
                return out, x.grad

            def unrolled(K):
                x = sos.clone().requires_grad_(True)
                out = s.forward(x, num_iterations=K, residuals="norms", checkpoint_every=25)
                loss(out["wavefields"][-1]).backward()
                return out, x.grad

            def adjoint_row(pre, out, t, spread, peak):
                return {"n": n, "batch": a.batch, "what": "adjoint solve alone", "absorption": a.absorption, "density": a.density, "precondition": pre, "tol": a.tol,
                        "restart": a.restart, "seconds": t, "seconds_spread": spread, "peak_torch_bytes": peak, "cycles": out["cycles"],
                        "lockstep_inner_iterations": out["iterations"], "operator_applications": out["operator_applications"],
                        "unet_evaluations": out["unet_evaluations"], "converged": bool(out["converged"]), "final_true_rmse": out["residual_norm"].tolist()}

            grads = {}
            for name, pre in (("learned", "learned"), ("plain", None)):
                (out, g), t, spread, peak, lib = _measure(lambda: implicit(pre), a.repeats)
                grads[name] = g
                info = out["adjoint"]
                rows.append({"n": n, "batch": a.batch, "what": "implicit", "absorption": a.absorption, "density": a.density, "precondition": pre, "tol": a.tol, "restart": a.restart, "seconds": t,
                             "seconds_spread": spread, "peak_torch_bytes": peak, "first_call_device_bytes": lib, "forward_cycles": len(out["cycle_tables"]),
                             "forward_converged": bool(out["converged"]), "forward_final_rmse": out["residual_norms"][-1].tolist(),
                             "forward_unet_evaluations": out["unet_evaluations"], "adjoint_cycles": info["cycles"], "adjoint_converged": bool(info["converged"]),
                             "adjoint_final_true_rmse": info["rmse"].tolist(), "adjoint_unet_evaluations": info["unet_evaluations"]})
                print(json.dumps(rows[-1]), flush=True)
                out, t, spread, peak, _ = _measure(lambda: s.adjoint_solve(cot, sos, restart=a.restart, max_outer=a.max_cycles, tol=a.tol, precondition=pre,
                                                                           **lossy), a.repeats)
                rows.append(adjoint_row(pre, out, t, spread, peak))
                print(json.dumps(rows[-1]), flush=True)
            if a.density:        # the learned preconditioner between W alone: the cycle is handed a plane of ones in rho's place
                out, t, spread, peak, _ = _measure(lambda: w_alone(s, sos, lossy, cot, a), a.repeats)
                rows.append(adjoint_row("learned, W alone", out, t, spread, peak))
                print(json.dumps(rows[-1]), flush=True)
            if lossy:
                continue
            target = max(rows[-4]["forward_final_rmse"])
            with torch.no_grad():
                norms = s.forward(sos, num_iterations=a.learned_iterations, residuals="norms")["residual_norms"].float().cpu().max(1).values
            below = (norms < target).nonzero()
            K = int(below[0]) + 1 if below.numel() else None
            (out, g), t, spread, peak, lib = _measure(lambda: unrolled(K or a.learned_iterations), a.repeats)
            rel = float((g - grads["learned"]).abs().max() / grads["learned"].abs().max())
            rows.append({"n": n, "batch": a.batch, "what": "unrolled forward(K, checkpoint_every=25) + backward", "target_rmse": target, "K": K,
                         "iterations_run": K or a.learned_iterations, "rmse_reached": float(out["residual_norms"][-1].detach().max()), "seconds": t, "seconds_spread": spread,
                         "peak_torch_bytes": peak, "first_call_device_bytes": lib, "max_rel_difference_to_implicit_gradient": rel,
                         "max_rel_difference_plain_to_learned_implicit": float((grads["plain"] - grads["learned"]).abs().max() / grads["learned"].abs().max())})
            print(json.dumps(rows[-1]), flush=True)
    props = torch.cuda.get_device_properties(0)
    text = json.dumps({"device": props.name, "hwmon": hw.summary(), "rows": rows}, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
