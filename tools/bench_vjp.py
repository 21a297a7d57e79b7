"""Cost of the solver's reverse mode (hn_step_vjp) next to the forward solve and the training step, on one GPU.

    python tools/bench_vjp.py [--iters 20] [--reps 3] [--sizes 256x32,512x16]

Per size (n^2 x batch): forward it/s plain (hn_step, nothing kept) and with the tape kept (the three histories written in place);
hn_step_vjp ms per iteration with and without the weight gradient (cotangent on the last wavefield), and with the weight gradient and
cotangents on every history entry; hn_train_grad(n_unroll = 1) ms per iteration.  Best of --reps
timed calls after one warm-up, CUDA events on the caller's stream.  Prints one line per size and a JSON line at the end.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helmnet_amd import IterativeSolver  # noqa: E402
from helmnet_amd.autograd import weight_blob  # noqa: E402
from helmnet_amd.phantoms import ring_sos_batch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="256x32,512x16")
    args = ap.parse_args()
    dev = "cuda:0"
    solver = IterativeSolver.from_exported_weights()
    solver.freeze()
    solver.to(dev)
    rows = []
    for spec in args.sizes.split(","):
        n, b = (int(x) for x in spec.split("x"))
        K = args.iters
        solver.set_domain_size(n, source_location=[n // 8, n // 2])
        eng = solver.engine()
        L = eng.state_len
        sos = torch.from_numpy(ring_sos_batch(n, b, seed=1)).to(dev)
        k_sq = ((1.0 / sos) ** 2).contiguous()
        src = solver.source.detach().contiguous()
        wf0 = torch.zeros(b, 2, n, n, device=dev)
        res0 = eng.residual(wf0, k_sq, src)
        st0 = torch.zeros(b, 2, L, device=dev)
        blob = weight_blob(solver.f).detach().contiguous()
        wh, rh, sh = torch.empty(K, b, 2, n, n, device=dev), torch.empty(K, b, 2, n, n, device=dev), torch.empty(K, b, 2, L, device=dev)

        def fwd(tape):
            wf, res, st = wf0.clone(), res0.clone(), st0.clone()
            eng.step(wf, res, st, k_sq, src, K, rh if tape else None, wh if tape else None, sh if tape else None)

        t_plain = timed(lambda: fwd(False), args.reps)
        t_tape = timed(lambda: fwd(True), args.reps)
        fwd(True)
        g_wf = torch.randn(b, 2, n, n, device=dev)
        g_k = torch.zeros_like(k_sq)
        g_w = torch.zeros_like(blob)
        t_vjp_w = timed(lambda: eng.step_vjp(blob, wf0, res0, st0, k_sq, 1, wh, rh, sh, g_wf_T=g_wf, g_k_sq=g_k, g_weights=g_w), args.reps)
        t_vjp = timed(lambda: eng.step_vjp(blob, wf0, res0, st0, k_sq, 1, wh, rh, sh, g_wf_T=g_wf, g_k_sq=g_k), args.reps)
        # a loss over every history entry: the seed kernel also reads the three cotangent histories
        gwh, grh, gsh = torch.randn_like(wh), torch.randn_like(rh), torch.randn_like(sh)
        t_vjp_h = timed(lambda: eng.step_vjp(blob, wf0, res0, st0, k_sq, 1, wh, rh, sh, gwh, grh, gsh, g_k_sq=g_k, g_weights=g_w), args.reps)
        del gwh, grh, gsh
        eng.train_reserve(b, 1)
        t_train = timed(lambda: eng.train_grad(blob, wf0, res0, st0, k_sq, src, 1), args.reps)
        row = {"n": n, "batch": b, "iters": K, "fwd_plain_it_s": K / t_plain * 1e3, "fwd_tape_it_s": K / t_tape * 1e3,
               "vjp_w_ms_per_it": t_vjp_w / K, "vjp_ms_per_it": t_vjp / K, "vjp_w_hist_ms_per_it": t_vjp_h / K, "train_grad_1_ms": t_train,
               "ratio_vjp_w_over_train": (t_vjp_w / K) / t_train, "ratio_vjp_w_hist_over_train": (t_vjp_h / K) / t_train}
        rows.append(row)
        print(f"{n}^2 x {b}: forward {row['fwd_plain_it_s']:.1f} it/s plain, {row['fwd_tape_it_s']:.1f} it/s with tape; "
              f"hn_step_vjp {row['vjp_w_ms_per_it']:.3f} ms/it with weights, {row['vjp_ms_per_it']:.3f} without, "
              f"{row['vjp_w_hist_ms_per_it']:.3f} with weights and cotangents on every history entry; "
              f"hn_train_grad(1) {t_train:.3f} ms; ratio {row['ratio_vjp_w_over_train']:.3f} ({row['ratio_vjp_w_hist_over_train']:.3f} with the histories)", flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
