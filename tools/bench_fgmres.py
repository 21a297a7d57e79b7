#!/usr/bin/env python
"""What the learned preconditioner buys restarted GMRES: cycles, inner iterations, operator applications, UNet evaluations and time to a tolerance.

    python tools/bench_fgmres.py [--out FILE]

Sweep at 96^2 (source [82, 48]) and 256^2 (source [194, 128]), batch 4, ring phantoms: restart in {10, 20}, precond_iterations m in {0, 1, 2, 5, 10},
alpha in {0.1, 1, 10} x the default (the source's RMS 2-norm); each configuration solved to 1e-4 in fp32 (``gmres(backend="hip",
precondition="learned")``) and to 1e-10 with the float64 refinement (``refine=True``).  m = 0 is the flexible cycle without a preconditioner (alpha
does not enter: one row).  Next to them the unpreconditioned ``gmres`` / ``gmres64`` and the learned solver alone to its floor (the smallest residual
RMSE of ``--learned-iterations`` iterations and where it is reached).

A solve is capped (``--max-cycles``, ``--max-unet``: cycles x restart x m): a row that hits its cap says ``converged: false`` with the residual it
reached, which is a measurement too.  Time: device events around the whole solve on the current stream, the driver's one host read per cycle
included (it is part of what a user waits for); one short warm-up solve, then the median of up to ``--repeats`` solves -- a solve longer than
``--budget`` seconds is not repeated (``repeats`` says how many were timed).  The true RMSE of every result is evaluated afterwards (fp32 solves:
``hn_residual`` + ``hn_rmse``; refined: ``hn_residual_f64``).  The shader clock is the median of the board's hwmon readings while the sweep runs
(bench.py's sampler), null where the board does not expose it."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) * 1e-3


def _ints(text):
    return [int(t) for t in text.split(",") if t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="96,256")
    ap.add_argument("--restarts", default="10,20")
    ap.add_argument("--iters", default="0,1,2,5,10")
    ap.add_argument("--scales", default="0.1,1,10")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=float, default=1.0)
    ap.add_argument("--max-cycles", type=int, default=1500)
    ap.add_argument("--max-unet", default="40000,12000", help="one cap for all sizes, or one per size")
    ap.add_argument("--learned-iterations", type=int, default=1000)
    ap.add_argument("--modes", default="fp32,refined")
    a = ap.parse_args()
    from bench import Hwmon
    from helmnet_amd import IterativeSolver
    from helmnet_amd.gmres import default_precond_scale, gmres
    from helmnet_amd.phantoms import ring_sos_batch
    dev = "cuda:0"
    tols = {"fp32": 1e-4, "refined": 1e-10}
    rows, learned = [], []
    hw = Hwmon(torch.device(dev))
    props = torch.cuda.get_device_properties(0)

    def write(final):
        result = {"device": props.name, "hwmon": hw.summary() if final else None, "complete": final,
                  "caps": {"sizes": a.sizes, "max_cycles": a.max_cycles, "max_unet": a.max_unet, "budget_s": a.budget}, "learned_alone": learned, "rows": rows}
        text = json.dumps(result, indent=1)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text + "\n")
        elif final:
            print(text)

    with hw:
        sizes, caps = _ints(a.sizes), _ints(a.max_unet)
        for n, max_unet in zip(sizes, caps * len(sizes) if len(caps) == 1 else caps):
            s = IterativeSolver.from_exported_weights(); s.freeze(); s.to(dev)
            s.set_domain_size(n, source_location=[82, 48] if n == 96 else [n - 62, n // 2])
            eng = s.engine()
            sos = torch.from_numpy(ring_sos_batch(n, a.batch, seed=11)).to(dev)
            k_sq = s.get_initials(sos)[0].contiguous()
            src = s.source.detach().float().contiguous()
            alpha0 = default_precond_scale(src)

            def true_rmse(out, mode):
                if mode == "refined":
                    return eng.residual64(out["wavefield"], k_sq.double(), src.double(), False, True)[1].tolist()
                return eng.rmse(eng.residual(out["wavefield"], k_sq, src)).tolist()

            def solve(mode, restart, m, scale, cycles):
                kw = {} if m is None else {"precondition": "learned", "precond_iterations": m, "precond_scale": scale * alpha0}
                return gmres(s, sos, restart=restart, max_outer=cycles, tol=tols[mode], backend="hip", refine=mode == "refined", **kw)

            # the learned solver alone
            s.forward(sos, num_iterations=10, residuals="norms")
            out, t = _event_timed(lambda: s.forward(sos, num_iterations=a.learned_iterations, residuals="norms"))
            norms = out["residual_norms"].float().cpu()                       # [K, B]
            worst = norms.max(1).values
            learned.append({"n": n, "batch": a.batch, "iterations": a.learned_iterations, "seconds": t, "floor_rmse_worst_sample": float(worst.min()),
                            "floor_at_iteration": int(worst.argmin()) + 1, "first_iteration_below_1e-4": int((worst < 1e-4).nonzero()[0]) + 1 if bool((worst < 1e-4).any()) else None,
                            "final_rmse": norms[-1].tolist()})
            for mode in [t for t in a.modes.split(",") if t]:
                for restart in _ints(a.restarts):
                    configs = [(None, None)] + [(m, sc) for m in _ints(a.iters) for sc in ([1.0] if m == 0 else [float(t) for t in a.scales.split(",")])]
                    for m, scale in configs:
                        cycles = a.max_cycles if not m else max(1, min(a.max_cycles, max_unet // (restart * m)))
                        solve(mode, restart, m, scale, 1)                    # warm: workspaces, tables, the stream probe
                        times, out = [], None
                        for _ in range(a.repeats):
                            out, t = _event_timed(lambda: solve(mode, restart, m, scale, cycles))
                            times.append(t)
                            if t > a.budget:
                                break
                        n_cycles = len(out["cycle_tables"])
                        rows.append({"n": n, "batch": a.batch, "mode": mode, "tol": tols[mode], "restart": restart,
                                     "precondition": None if m is None else "learned", "precond_iterations": m, "alpha_over_default": scale,
                                     "alpha": None if m is None else scale * alpha0, "cycles": n_cycles, "cycle_cap": cycles,
                                     "lockstep_inner_iterations": out["iterations"], "operator_applications": out["operator_applications"],
                                     "operator_applications64": out.get("operator_applications64"), "unet_evaluations": out["unet_evaluations"],
                                     "seconds": statistics.median(times), "seconds_spread": [min(times), max(times)], "repeats": len(times),
                                     "converged": bool(out["converged"]), "final_true_rmse": true_rmse(out, mode)})
                        print(json.dumps(rows[-1]), flush=True)
                        write(False)                                          # a sweep that is cut off keeps what it measured
    write(True)


if __name__ == "__main__":
    main()
