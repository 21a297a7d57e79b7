"""Reverse mode through the solver: ``torch.autograd.Function``s over the library's entry points.

The reference's solver is plain PyTorch, so autograd flows through ``IterativeSolver.forward`` / ``n_steps`` / ``single_step`` /
``get_residual`` / ``apply_laplacian`` (hybridnet.py:522-584, 586-623, 654-697).  Here those run in libhelmnet_hip.so, and these
Functions supply the backward passes:

  * ``Laplacian``   L(x);                        backward L^H(g)             (hn_residual_vjp with k_sq = 0)
  * ``Residual``    L(wf) + k_sq wf - src;       backward w.r.t. wf (hn_residual_vjp), k_sq and src
  * ``Solve``       K iterations of hn_step;     backward hn_step_vjp, the forward's histories being the tape (every ``checkpoint_every``-th
                    state kept and the segments in between re-run with hn_step when c > 1: the same bits as c = 1)
  * ``SolveImplicit``  the wavefield a linear solve converged to (IterativeSolver.solve_implicit); backward by the adjoint-state method: one solve
                    of A^H lam = g (gmres_adjoint) and hn_adjoint_grad, nothing taped; no forward mode

The weight blob the kernels read is assembled from the network's parameters with torch ops (``weight_blob``), so the blob gradient
lands on each ``nn.Parameter`` and the zero padding of levels without state gets none.  No double backward: a backward pass
recorded with ``create_graph=True`` raises.

Forward mode (``torch.autograd.forward_ad``): each Function also has a ``jvp``.  ``Laplacian.jvp`` is L of the tangent, ``Residual.jvp``
L(wf') + k_sq wf' + k_sq' wf - src', ``Solve.jvp`` hn_step_jvp over the same tape (segments re-run with hn_step when c > 1).  The weights
are constants of the linearisation: a tangent on the weight blob raises NotImplementedError.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from . import _lib
from .engine import weight_names

_CONST_SLOPE = {"relu": 0.0, "leakyrelu": 0.01, "celu": 0.0, "tanh": 0.0, "gelu": 0.0, "tanhshrink": 0.0, "softplus": 0.0}
_ZERO_STATE_DC = {"0.weight": 2 * 10 * 9, "0.bias": 2, "2.weight": 2 * 2 * 9, "2.bias": 2}


def weight_blob(f) -> torch.Tensor:
    """The fp32 blob of hn_load_weights (engine.pack_weights order and padding) built from ``f``'s parameters with torch ops: its
    gradient flows back onto the parameters.  Constant slopes of parameter-free activations and the zero padding of levels without
    state (d >= state_depth) are constants."""
    params = dict(f.named_parameters())
    dev = next(f.parameters()).device
    act = f.activation_function.lower()
    stateless = {f"enc.{d}." for d in range(f.state_depth, f.depth)}
    const = lambda v: torch.full((1,), v, device=dev, dtype=torch.float32)  # noqa: E731
    parts = []
    for name in weight_names(f.depth):
        level = name[: name.index(".", 4) + 1] if name.startswith("enc.") else None
        if level in stateless and ".conv_state." in name:
            tail = name.split(".double_conv.")[1]
            parts.append(const(0.25) if tail == "1.weight" else torch.zeros(_ZERO_STATE_DC[tail], device=dev, dtype=torch.float32))
            continue
        if name.endswith(".double_conv.1.weight") and name not in params:
            if act not in _CONST_SLOPE:
                raise KeyError(f"missing {name} for activation {act!r}")
            parts.append(const(_CONST_SLOPE[act]))
            continue
        v = params[name].float()
        if level in stateless and name.endswith(".conv_signal.double_conv.0.weight"):
            v = torch.cat([v, v.new_zeros(v.shape[0], 2, 3, 3)], 1)
        parts.append(v.reshape(-1))
    return torch.cat(parts)


def rmse_cotangent(g_rmse: torch.Tensor, res: torch.Tensor, rmse: torch.Tensor) -> torch.Tensor:
    """Residual cotangent of rmse = sqrt(mean_{c,h,w} res^2) (test_loss_function, hybridnet.py:295-297): g * res / (numel * rmse),
    per leading index.  g_rmse / rmse [..., B], res [..., B, 2, n, n]."""
    numel = res.shape[-3] * res.shape[-2] * res.shape[-1]
    scale = g_rmse / (numel * rmse)
    return scale[..., None, None, None] * res


def _no_double_backward():
    if torch.is_grad_enabled():
        raise RuntimeError("helmnet_amd: the solver's backward pass is not differentiable (create_graph=True / double backward is not supported)")


class Laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, x):
        ctx.eng = eng
        return eng.laplacian(x.detach().contiguous())

    @staticmethod
    def backward(ctx, g):
        _no_double_backward()
        eng = ctx.eng
        g = g.contiguous()
        zero = torch.zeros(g.shape[0], 1, g.shape[2], g.shape[3], device=g.device, dtype=torch.float32)
        return None, eng.residual_vjp(g, zero)

    @staticmethod
    def jvp(ctx, _eng, t_x):
        return ctx.eng.laplacian(t_x.float().contiguous())


class Residual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, wf, k_sq, src):
        wf, k_sq, src = wf.detach().contiguous(), k_sq.detach().contiguous(), src.detach().contiguous()
        ctx.eng, ctx.src_batch = eng, src.shape[0]
        ctx.save_for_backward(wf, k_sq)
        ctx.save_for_forward(wf, k_sq)
        return eng.residual(wf, k_sq, src)

    @staticmethod
    def backward(ctx, g):
        _no_double_backward()
        wf, k_sq = ctx.saved_tensors
        g = g.contiguous()
        g_wf = ctx.eng.residual_vjp(g, k_sq) if ctx.needs_input_grad[1] else None
        g_k = (g * wf).sum(1, keepdim=True) if ctx.needs_input_grad[2] else None
        g_s = None
        if ctx.needs_input_grad[3]:
            g_s = -g if ctx.src_batch == g.shape[0] else -g.sum(0, keepdim=True)
        return None, g_wf, g_k, g_s

    @staticmethod
    def jvp(ctx, _eng, t_wf, t_k, t_s):
        wf, k_sq = ctx.saved_tensors
        s_tilde = (t_s.float() - t_k.float() * wf).contiguous()   # [B, 2, n, n]: the residual of the tangent with this source is the whole tangent
        return ctx.eng.residual(t_wf.float().contiguous(), k_sq, s_tilde)


def rmse_tangent(t_res: torch.Tensor, res: torch.Tensor, rmse: torch.Tensor) -> torch.Tensor:
    """Tangent of rmse = sqrt(mean_{c,h,w} res^2): <res, t_res> / (numel * rmse), per leading index (the transpose of ``rmse_cotangent``)."""
    numel = res.shape[-3] * res.shape[-2] * res.shape[-1]
    return (res * t_res).sum((-3, -2, -1)) / (numel * rmse)


class SolveSpec:
    """What a Solve call needs besides its tensor inputs."""

    def __init__(self, eng, num_iterations: int, checkpoint_every: int, keep_wf: bool, keep_res: bool, keep_st: bool,
                 stateless: List[Tuple[int, int]]):
        if checkpoint_every < 1:
            raise ValueError(f"checkpoint_every must be >= 1, got {checkpoint_every}")
        self.eng, self.K, self.c = eng, int(num_iterations), int(checkpoint_every)
        self.keep_wf, self.keep_res, self.keep_st = keep_wf, keep_res, keep_st
        self.stateless = list(stateless)


class Solve(torch.autograd.Function):
    """(wf0, res0, states0, k_sq, src, blob) -> (wavefields, residuals, states, rmse) of K solver iterations.  The first three outputs are the
    whole history [K, ...] where the spec keeps it, else the last entry [1, ...]; rmse is [K, B].  With checkpoint_every == 1 the three
    histories are kept (they are the tape, even with residuals='norms'); with c > 1 only (wf, res, states) in front of every c-th
    iteration, and backward re-runs each segment with hn_step before hn_step_vjp."""

    @staticmethod
    def forward(ctx, spec: SolveSpec, wf0, res0, st0, k_sq, src, blob):
        eng, K, c = spec.eng, spec.K, spec.c
        b, n, L = wf0.shape[0], eng.n, eng.state_len
        dev = wf0.device
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
        wf, res = wf0.detach().float().clone().contiguous(), res0.detach().float().clone().contiguous()
        st = st0.detach().float().clone().contiguous()
        for a, e in spec.stateless:   # levels without state: zeros into the kernels, the caller's values back out (HybridNet.to_engine_states)
            st[:, :, a:e] = 0
        st_in = st.clone()
        ksq, srcd, blobd = k_sq.detach().contiguous(), src.detach().float().contiguous(), blob.detach().contiguous()
        rmse = new(K, b)
        ck = []
        if c == 1:
            wf_out, res_out, st_out = new(K, b, 2, n, n), new(K, b, 2, n, n), new(K, b, 2, L)
            eng.step(wf, res, st, ksq, srcd, K, res_out, wf_out, st_out, rmse)
            tape = (wf_out, res_out, st_out)
        else:
            wf_out = new(K, b, 2, n, n) if spec.keep_wf else None
            res_out = new(K, b, 2, n, n) if spec.keep_res else None
            st_out = new(K, b, 2, L) if spec.keep_st else None
            for s0 in range(0, K, c):
                s1 = min(s0 + c, K)
                ck.append((wf.clone(), res.clone(), st.clone()))
                seg = lambda out, *shape: out[s0:s1] if out is not None else new(s1 - s0, *shape)  # noqa: E731
                eng.step(wf, res, st, ksq, srcd, s1 - s0, seg(res_out, b, 2, n, n), seg(wf_out, b, 2, n, n), seg(st_out, b, 2, L), rmse[s0:s1])
            tape = None
            wf_out = wf_out if wf_out is not None else wf[None]
            res_out = res_out if res_out is not None else res[None]
            st_out = st_out if st_out is not None else st[None]
        if c == 1:
            if not spec.keep_wf:
                wf_out = wf_out[K - 1:]
            if not spec.keep_res:
                res_out = res_out[K - 1:]
            if not spec.keep_st:
                st_out = st_out[K - 1:]
        outs = [wf_out, res_out, st_out.clone() if spec.stateless else st_out]
        for a, e in spec.stateless:
            outs[2][..., a:e] = st0.detach()[:, :, a:e]
        # everything backward reads goes through save_for_backward: a tape tensor that is also an output (or shares its storage) and is
        # modified in place by the caller makes backward raise instead of linearising around the modified values
        ctx.spec, ctx.src_batch, ctx.n_ck = spec, srcd.shape[0], len(ck)
        saved = (wf0.detach().float().contiguous(), res0.detach().float().contiguous(), st_in, ksq, blobd, rmse, srcd,
                 *(tape if tape is not None else ()), *(t for trip in ck for t in trip))
        ctx.save_for_backward(*saved)
        ctx.save_for_forward(*saved)
        ctx.set_materialize_grads(False)
        return outs[0], outs[1], outs[2], rmse

    @staticmethod
    def backward(ctx, g_wf, g_res, g_st, g_rmse):
        _no_double_backward()
        spec, eng = ctx.spec, ctx.spec.eng
        K, c = spec.K, spec.c
        saved = ctx.saved_tensors
        wf0, res0, st0, ksq, blob, rmse, srcd = saved[:7]
        tape = saved[7:10] if c == 1 else None
        ck = [saved[7 + 3 * j: 10 + 3 * j] for j in range(ctx.n_ck)]
        src_batch = ctx.src_batch
        b, n, L = wf0.shape[0], eng.n, eng.state_len
        dev = wf0.device
        need = ctx.needs_input_grad
        g_k = torch.zeros_like(ksq) if need[4] else None
        g_s = torch.zeros(src_batch, 2, n, n, device=dev, dtype=torch.float32) if need[5] else None
        g_w = torch.zeros_like(blob) if need[6] else None
        cont = lambda t: None if t is None else t.float().contiguous()  # noqa: E731
        g_wf, g_res, g_st, g_rmse = cont(g_wf), cont(g_res), cont(g_st), cont(g_rmse)
        # cotangents on the last outputs where only the last entry is an output
        g_wf_T = g_wf[0] if (g_wf is not None and not spec.keep_wf) else None
        g_res_T = g_res[0] if (g_res is not None and not spec.keep_res) else None
        g_st_T = g_st[0] if (g_st is not None and not spec.keep_st) else None
        # levels without state pass their slot through unchanged: the cotangent is the identity (added at the end)
        ident = None
        if spec.stateless:
            ident = torch.zeros_like(st0)
            if g_st is not None:
                src_st = g_st.sum(0) if spec.keep_st else g_st[0]
                for a, e in spec.stateless:
                    ident[:, :, a:e] = src_st[:, :, a:e]
                g_st = g_st.clone()
                for a, e in spec.stateless:
                    g_st[..., a:e] = 0
                if g_st_T is not None:
                    g_st_T = g_st[0]
        segs = [(0, K)] if c == 1 else [(s0, min(s0 + c, K)) for s0 in range(0, K, c)]
        for j in range(len(segs) - 1, -1, -1):
            s0, s1 = segs[j]
            if c == 1:
                wf_t, res_t, st_t = tape
                start = (wf0, res0, st0)
            else:   # re-run the segment from its checkpoint: hn_step is deterministic, so this is the forward's tape bit for bit
                start = ck[j]
                m = s1 - s0
                wf_t, res_t, st_t = (torch.empty(m, b, 2, n, n, device=dev), torch.empty(m, b, 2, n, n, device=dev), torch.empty(m, b, 2, L, device=dev))
                wf, res, st = (t.clone() for t in start)
                eng.step(wf, res, st, ksq, srcd, m, res_t, wf_t, st_t, torch.empty(m, b, device=dev))
            if spec.stateless:   # the kernels saw zeros in the stateless slots
                st_t = st_t.clone()
                for a, e in spec.stateless:
                    st_t[..., a:e] = 0
            gw = g_wf[s0:s1] if (g_wf is not None and spec.keep_wf) else None
            gr = g_res[s0:s1] if (g_res is not None and spec.keep_res) else None
            gs = g_st[s0:s1] if (g_st is not None and spec.keep_st) else None
            if g_rmse is not None:
                rc = rmse_cotangent(g_rmse[s0:s1], res_t, rmse[s0:s1])
                gr = rc if gr is None else (gr + rc)
            flags = (_lib.HN_VJP["continue"] if j < len(segs) - 1 else 0) | (_lib.HN_VJP["defer"] if j > 0 else 0)
            out = eng.step_vjp(blob, start[0], start[1], start[2], ksq, src_batch, wf_t, res_t, st_t,
                               cont(gw), cont(gr), cont(gs), g_wf_T, g_res_T, g_st_T, g_k, g_s, g_w, flags)
            g_wf_T, g_res_T, g_st_T = out["grad_wf"], out["grad_res"], out["grad_states"]
        if ident is not None:
            for a, e in spec.stateless:
                g_st_T[:, :, a:e] = ident[:, :, a:e]
        return (None, g_wf_T if need[1] else None, g_res_T if need[2] else None, g_st_T if need[3] else None, g_k, g_s, g_w)

    @staticmethod
    def jvp(ctx, _spec, t_wf0, t_res0, t_st0, t_k, t_s, t_blob):
        """Tangents of the four outputs: hn_step_jvp over the tape the forward kept, or (c > 1) over each segment re-run from its checkpoint."""
        if t_blob is not None:
            raise NotImplementedError("helmnet_amd: forward mode has no weight tangents: the weights are constants of the linearisation "
                                      "(hn_step_jvp); take weight derivatives in reverse mode")
        spec, eng = ctx.spec, ctx.spec.eng
        K, c = spec.K, spec.c
        saved = ctx.saved_tensors
        wf0, res0, st0, ksq, _blob, rmse, _srcd = saved[:7]
        tape = saved[7:10] if c == 1 else None
        ck = [saved[7 + 3 * j: 10 + 3 * j] for j in range(ctx.n_ck)]
        b, n, L = wf0.shape[0], eng.n, eng.state_len
        dev = wf0.device
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
        own = lambda t, like: torch.zeros_like(like) if t is None else t.detach().float().clone().contiguous()  # noqa: E731
        t_wf, t_res, t_st = own(t_wf0, wf0), own(t_res0, res0), own(t_st0, st0)
        ident = t_st.clone() if spec.stateless else None   # levels without state pass their slot through unchanged: so does its tangent
        for a, e in spec.stateless:
            t_st[:, :, a:e] = 0
        t_k = None if t_k is None else t_k.detach().float().contiguous()
        t_s = None if t_s is None else t_s.detach().float().contiguous()
        t_wf_h = new(K, b, 2, n, n) if spec.keep_wf else None
        t_st_h = new(K, b, 2, L) if spec.keep_st else None
        t_res_h = new(K, b, 2, n, n) if spec.keep_res else None
        t_rmse = new(K, b)
        segs = [(0, K)] if c == 1 else [(s0, min(s0 + c, K)) for s0 in range(0, K, c)]
        for j, (s0, s1) in enumerate(segs):
            if c == 1:
                wf_t, res_t, st_t = tape
                start = (wf0, res0, st0)
            else:   # re-run the segment from its checkpoint: hn_step is deterministic, so this is the forward's tape bit for bit
                start = ck[j]
                m = s1 - s0
                wf_t, res_t, st_t = new(m, b, 2, n, n), new(m, b, 2, n, n), new(m, b, 2, L)
                wf, res, st = (t.clone() for t in start)
                eng.step(wf, res, st, ksq, _srcd, m, res_t, wf_t, st_t, new(m, b))
            if spec.stateless:   # the kernels saw zeros in the stateless slots
                st_t = st_t.clone()
                for a, e in spec.stateless:
                    st_t[..., a:e] = 0
            seg = lambda h: None if h is None else h[s0:s1]  # noqa: E731
            t_res_seg = seg(t_res_h) if spec.keep_res else new(s1 - s0, b, 2, n, n)   # every iteration's residual tangent feeds the rmse tangent
            eng.step_jvp(start[0], start[1], start[2], ksq, ctx.src_batch, wf_t, res_t, st_t, t_wf, t_res, t_st, t_k, t_s,
                         seg(t_wf_h), t_res_seg, seg(t_st_h))
            t_rmse[s0:s1] = rmse_tangent(t_res_seg, res_t, rmse[s0:s1])
        out_wf = t_wf_h if spec.keep_wf else t_wf[None]
        out_res = t_res_h if spec.keep_res else t_res[None]
        out_st = t_st_h if spec.keep_st else t_st[None]
        for a, e in spec.stateless:
            out_st[..., a:e] = ident[:, :, a:e]
        return out_wf, out_res, out_st, t_rmse


# ---- adjoint-state gradients of a converged linear solve (IterativeSolver.solve_implicit) ----
def adjoint_state_grads(lam: torch.Tensor, u: torch.Tensor, sos: torch.Tensor, omega: float, g_k_sq: torch.Tensor = None):
    """The chain rule of the adjoint-state method, in the tensors' own dtype (float64 on the host in the tests, fp32 on the device in
    ``SolveImplicit``).  With A u = src, A u = L(u) + k_sq * u, k_sq = (omega / sos)^2, a real loss J and A^H lam = dJ/du (fields as two real planes
    [B,2,n,n]): dJ = Re<lam, dsrc - dk_sq * u>, hence dJ/dsrc = lam, dJ/dk_sq = -Re(conj(lam) u) = -(lam_re u_re + lam_im u_im) and
    dJ/dsos = dJ/dk_sq * (-2 omega^2 / sos^3).  ``g_k_sq`` [B,1,n,n]: dJ/dk_sq when the caller has it already (hn_adjoint_grad), else it is formed
    here.  Returns (g_sos [B,1,n,n], g_k_sq); the per-sample source gradient is ``lam`` itself."""
    if g_k_sq is None:
        g_k_sq = -(lam * u).sum(1, keepdim=True)
    return g_k_sq * (-2.0 * float(omega) ** 2 / sos ** 3), g_k_sq


class SolveImplicit(torch.autograd.Function):
    """(sos, src) -> the wavefield a forward solve converged to, whichever route converged it; backward is the adjoint-state method: one solve of
    A^H lam = g (gmres_adjoint), hn_adjoint_grad and the chain rule -- O(1) memory, nothing of the forward solve is taped.  ``spec``: solver, the
    converged wavefield, the adjoint solve's keyword arguments and ``info``, the dictionary the backward pass fills (cycles, rmse, converged)."""

    @staticmethod
    def forward(ctx, spec, sos, src):
        ctx.spec, ctx.src_batch, ctx.adjoint_info = spec, src.shape[0], spec["info"]
        ctx.save_for_backward(sos.detach())
        return spec["wavefield"].clone()

    @staticmethod
    def backward(ctx, g):
        _no_double_backward()
        from .gmres import gmres_adjoint
        spec = ctx.spec
        (sos,) = ctx.saved_tensors
        solver, u = spec["solver"], spec["wavefield"]
        with torch.no_grad():
            adj = gmres_adjoint(solver, sos, g.detach().float().contiguous(), **spec["adjoint_kwargs"])
            lam = adj["wavefield"]
            g_k_sq, g_src = solver.engine().adjoint_grad(lam, u, ctx.src_batch if ctx.needs_input_grad[2] else None)
            g_sos = adjoint_state_grads(lam, u, sos, float(solver.hparams.omega), g_k_sq)[0] if ctx.needs_input_grad[1] else None
        ctx.adjoint_info.update({"cycles": adj["cycles"], "rmse": adj["residual_norm"], "converged": adj["converged"], "iterations": adj["iterations"],
                             "unet_evaluations": adj["unet_evaluations"]})
        return None, g_sos, g_src


class SolveImplicitLossy(torch.autograd.Function):
    """``SolveImplicit`` for an absorbing medium: (sos, alpha, src) -> the converged wavefield of A u = L(u) + (k_sq + i k_sq_im) u = src, the two
    planes from ``absorption.complex_k_sq``.  backward solves A^H lam = g on the lossy adjoint (gmres_adjoint with ``absorption``), forms dJ/dk_sq,
    dJ/dk_sq_im and dJ/dsrc in one launch (hn_adjoint_grad_lossy) and applies ``absorption.complex_k_sq_grads``; the gradient of ``alpha`` is summed
    over the dimensions it was broadcast along."""

    @staticmethod
    def forward(ctx, spec, sos, alpha, src):
        ctx.spec, ctx.src_batch, ctx.adjoint_info = spec, src.shape[0], spec["info"]
        ctx.save_for_backward(sos.detach(), alpha.detach())
        return spec["wavefield"].clone()

    @staticmethod
    def backward(ctx, g):
        _no_double_backward()
        from .absorption import complex_k_sq_grads
        from .gmres import gmres_adjoint
        spec = ctx.spec
        sos, alpha = ctx.saved_tensors
        solver, u = spec["solver"], spec["wavefield"]
        with torch.no_grad():
            adj = gmres_adjoint(solver, sos, g.detach().float().contiguous(), absorption=alpha, **spec["adjoint_kwargs"])
            lam = adj["wavefield"]
            g_k_sq, g_k_sq_im, g_src = solver.engine().adjoint_grad_lossy(lam, u, ctx.src_batch if ctx.needs_input_grad[3] else None)
            g_sos = g_alpha = None
            if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
                g_sos, g_alpha = complex_k_sq_grads(g_k_sq, g_k_sq_im, sos, alpha, float(solver.hparams.omega))
                g_sos = g_sos if ctx.needs_input_grad[1] else None
                g_alpha = (g_alpha.sum_to_size(alpha.shape) if alpha.dim() else g_alpha.sum()) if ctx.needs_input_grad[2] else None
        ctx.adjoint_info.update({"cycles": adj["cycles"], "rmse": adj["residual_norm"], "converged": adj["converged"], "iterations": adj["iterations"],
                                 "unet_evaluations": adj["unet_evaluations"]})
        return None, g_sos, g_alpha, g_src


class SolveImplicitMedium(torch.autograd.Function):
    """``SolveImplicitLossy`` for a medium of heterogeneous density, with absorption (``spec["lossy"]``) or without (``alpha`` is then a placeholder
    and gets no gradient): (sos, alpha, rho, src) -> the converged wavefield of A_rho u = src.  backward solves A_rho^H lam = g (gmres_adjoint with
    ``density``), forms dJ/dk_sq, dJ/dk_sq_im, dJ/dq and dJ/dsrc in one call (hn_adjoint_grad_medium) and chains: to ``sos`` and ``alpha`` through
    ``absorption.complex_k_sq_grads`` (without absorption: the lossless chain of ``adjoint_state_grads``), to ``rho`` through
    ``density.log_density_gradient_vjp`` -- q does not enter its own gradient, dJ/dq = Re(conj(lam) b D u) per axis -- summed to rho's own shape."""

    @staticmethod
    def forward(ctx, spec, sos, alpha, rho, src):
        ctx.spec, ctx.src_batch, ctx.adjoint_info = spec, src.shape[0], spec["info"]
        ctx.save_for_backward(sos.detach(), alpha.detach(), rho.detach())
        return spec["wavefield"].clone()

    @staticmethod
    def backward(ctx, g):
        _no_double_backward()
        from .absorption import complex_k_sq_grads
        from .density import log_density_gradient_vjp
        from .gmres import gmres_adjoint
        spec = ctx.spec
        sos, alpha, rho = ctx.saved_tensors
        solver, u, lossy = spec["solver"], spec["wavefield"], spec["lossy"]
        need = ctx.needs_input_grad
        with torch.no_grad():
            medium = {"absorption": alpha, "density": rho} if lossy else {"density": rho}
            adj = gmres_adjoint(solver, sos, g.detach().float().contiguous(), **medium, **spec["adjoint_kwargs"])
            lam = adj["wavefield"]
            g_k_sq, g_k_sq_im, g_q, g_src = solver.engine().adjoint_grad_medium(lam, u, ctx.src_batch if need[4] else None, lossy)
            g_sos = g_alpha = g_rho = None
            if lossy and (need[1] or need[2]):
                g_sos, g_alpha = complex_k_sq_grads(g_k_sq, g_k_sq_im, sos, alpha, float(solver.hparams.omega))
                g_sos = g_sos if need[1] else None
                g_alpha = (g_alpha.sum_to_size(alpha.shape) if alpha.dim() else g_alpha.sum()) if need[2] else None
            elif need[1]:
                g_sos = adjoint_state_grads(lam, u, sos, float(solver.hparams.omega), g_k_sq)[0]
            if need[3]:
                g_rho = log_density_gradient_vjp(g_q, rho.expand(g_q.shape[0], 1, *g_q.shape[2:])).sum_to_size(rho.shape)
        ctx.adjoint_info.update({"cycles": adj["cycles"], "rmse": adj["residual_norm"], "converged": adj["converged"], "iterations": adj["iterations"],
                                 "unet_evaluations": adj["unet_evaluations"]})
        return None, g_sos, g_alpha, g_rho, g_src
