"""Cost of the solver's forward mode (hn_step_jvp) next to the plain iteration (hn_step) and the reverse mode without weight gradients (hn_step_vjp
without g_weights), on one GPU.

    python tools/bench_jvp.py [--iters 10] [--calls 7] [--sizes 96x8,256x8] [--out profiles/jvp_bench.json]

Per size (n^2 x batch): median over --calls timed calls of --iters iterations each (device events on the caller's stream) after one warm-up call of every
path (it builds the workspaces), the three paths alternating call by call so that all see the same clocks.  hn_step writes the three histories (the tape the
other two read); hn_step_jvp carries a direction on every input and no tangent history; hn_step_vjp a cotangent on the last wavefield.  The shader
clock is the median of the board's hwmon readings while the sweep runs.  Shipped weights, ring phantoms, the solver's point source.  A record of what
forward mode costs relative to the two existing loops on the same box: no bar."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--sizes", default="96x8,256x8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from bench import Hwmon
    from helmnet_amd import IterativeSolver
    from helmnet_amd.autograd import weight_blob
    from helmnet_amd.phantoms import ring_sos_batch
    dev = torch.device("cuda:0")
    solver = IterativeSolver.from_exported_weights()
    solver.freeze()
    solver.to(dev)
    hw, rows, T = Hwmon(dev), [], args.iters
    with hw:
        for size in args.sizes.split(","):
            n, b = (int(v) for v in size.split("x"))
            solver.set_domain_size(n, source_location=[n - n // 7, n // 2])
            eng = solver.engine()
            sos = torch.from_numpy(ring_sos_batch(n, b, seed=n)).to(dev)
            k_sq, wf0 = solver.get_initials(sos)
            k_sq, src = k_sq.contiguous(), solver._src()
            res0 = eng.residual(wf0, k_sq, src)
            st0 = torch.zeros(b, 2, eng.state_len, device=dev)
            blob = weight_blob(solver.f).detach().contiguous()
            new = lambda *shape: torch.empty(shape, device=dev)  # noqa: E731
            wh, rh, sh = new(T, b, 2, n, n), new(T, b, 2, n, n), new(T, b, 2, eng.state_len)
            g = torch.Generator(device=dev).manual_seed(n)
            rnd = lambda *shape: torch.randn(shape, device=dev, generator=g)  # noqa: E731
            t_k, t_s, g_wf = 0.1 * rnd(b, 1, n, n), rnd(*src.shape), rnd(b, 2, n, n)
            t_wf, t_res, t_st = new(b, 2, n, n), new(b, 2, n, n), new(b, 2, eng.state_len)

            def step():
                eng.step(wf0.clone(), res0.clone(), st0.clone(), k_sq, src, T, rh, wh, sh)

            def jvp():
                t_wf.zero_(); t_res.zero_(); t_st.zero_()
                eng.step_jvp(wf0, res0, st0, k_sq, src.shape[0], wh, rh, sh, t_wf, t_res, t_st, t_k, t_s)

            def vjp():
                eng.step_vjp(blob, wf0, res0, st0, k_sq, src.shape[0], wh, rh, sh, g_wf_T=g_wf)

            paths = {"step": step, "jvp": jvp, "vjp": vjp}
            times = {k: [] for k in paths}
            for call in range(args.calls + 1):          # call 0 warms up (and builds the workspaces)
                for name, fn in paths.items():
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    fn()
                    e.record()
                    e.synchronize()
                    if call > 0:
                        times[name].append(a.elapsed_time(e) / T)
            med = {k: statistics.median(v) for k, v in times.items()}
            rows.append({"n": n, "batch": b, "iterations_per_call": T, "calls": args.calls, "step_ms_per_it": med["step"], "jvp_ms_per_it": med["jvp"],
                         "vjp_ms_per_it": med["vjp"], "spread_ms": {k: [min(v), max(v)] for k, v in times.items()},
                         "jvp_over_step": med["jvp"] / med["step"], "jvp_over_vjp": med["jvp"] / med["vjp"]})
            print(json.dumps(rows[-1]), flush=True)
    result = {"device": torch.cuda.get_device_properties(0).name, "hwmon": hw.summary(), "what": "ms per solver iteration: hn_step (writing the three histories), "
              "hn_step_jvp (directions on k_sq and the source, no tangent history), hn_step_vjp without g_weights (cotangent on the last wavefield)", "rows": rows}
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
