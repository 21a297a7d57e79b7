"""Drop-in replacement for the reference's ``IterativeSolver`` inference API on MI355X.

Mirrors reference helmnet/hybridnet.py (inference half): ``load_from_checkpoint`` (Lightning
classmethod, re-implemented without Lightning), ``hparams``, ``freeze``, ``device``, ``to``,
``set_domain_size`` (:92-108), ``set_laplacian`` (:110-131), ``setup_source / set_source /
set_source_maps / set_multiple_sources / reset_source`` (:133-170), ``get_initials``
(:522-538), ``apply_laplacian`` (:540-542), ``get_residual`` (:544-556), ``single_step``
(:558-584), ``n_steps`` (:586-623), ``forward`` (:654-697), ``forward_variable_src``
(:699-754), ``test_loss_function`` (:295-297), ``loss_function`` (:285-293).  The training half (replay buffer,
``training_step``, optimiser, scheduler) lives in ``helmnet_amd.training`` (``solver.trainer()``), on ``hn_train_grad`` /
``hn_adam_step``; Lightning's hooks and TensorBoard logging have no counterpart.

All per-iteration arithmetic runs in libhelmnet_hip.so: ``forward`` / ``n_steps`` hand the whole
loop to ``hn_step`` (fused HIP kernels), ``get_residual`` to ``hn_residual``, ``f`` to ``hn_unet``.
``forward64`` / ``n_steps64`` / ``deviation_from_float64`` (extension) run the same loop in float64 on ``hn_step_f64``: the reference's
``solver.double()`` trajectory, to measure the other precision modes against.
``jvp`` / ``linearize`` (extension) are the solver's forward mode on ``hn_step_jvp``: directional derivatives with respect to the sound-speed
map and the source, O(chunk) memory.
There is no CPU path: a solver left on the CPU raises as soon as it is asked to compute.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from .checkpoint import AttributeDict, read_lightning_checkpoint
from .engine import Engine, Medium, _require_no_grad
from .laplacian import FastLaplacianWithPML, domain_hw
from .source import SourceModule
from .unet import HybridNet


def jvp_initial_tangents(omega: float, sos: torch.Tensor, d_sos: Optional[torch.Tensor], d_source: Optional[torch.Tensor]):
    """Tangents of ``get_initials`` and of the first residual along (d_sos, d_source): k_sq = (omega / sos)^2 gives
    k_sq' = -2 omega^2 sos' / sos^3; the wavefield starts at zero, so wf0' = 0 and res0' = L(0) + k_sq' . 0 - src' = -src'.
    Returns (t_k_sq or None, t_wf0, t_res0) with t_wf0 / t_res0 [B, 2, n, n]."""
    b, n = sos.shape[0], sos.shape[-1]
    t_k = None if d_sos is None else (-2.0 * omega ** 2 * d_sos / sos ** 3).contiguous()
    t_wf = torch.zeros(b, 2, n, n, device=sos.device, dtype=sos.dtype)
    t_res = t_wf.clone() if d_source is None else (-d_source).expand(b, 2, n, n).contiguous()
    return t_k, t_wf, t_res


def jvp_chunks(eng, wf, res, st, k_sq, src, t_wf, t_res, t_st, t_k, t_src, num_iterations: int, chunk: int):
    """Primal and tangent interleaved, ``chunk`` iterations at a time: ``eng.step`` into a chunk-slot history, then ``eng.step_jvp`` over it with
    the (wf, res, states) in front of the chunk as its linearisation start.  Every tensor but k_sq / src / t_k / t_src is updated in place;
    memory is O(chunk) whatever ``num_iterations`` is.  Returns the per-sample RMSE of the last iteration, [B]."""
    K, c = int(num_iterations), max(1, min(int(chunk), int(num_iterations)))
    b = wf.shape[0]
    new = lambda *shape: torch.empty(shape, device=wf.device, dtype=torch.float32)  # noqa: E731
    wf_h, res_h, st_h, rmse = new(c, *wf.shape), new(c, *res.shape), new(c, *st.shape), new(c, b)
    last = None
    for s0 in range(0, K, c):
        m = min(c, K - s0)
        start = (wf.clone(), res.clone(), st.clone())
        eng.step(wf, res, st, k_sq, src, m, res_h[:m], wf_h[:m], st_h[:m], rmse[:m])
        eng.step_jvp(start[0], start[1], start[2], k_sq, src.shape[0], wf_h[:m], res_h[:m], st_h[:m], t_wf, t_res, t_st, t_k, t_src)
        last = rmse[m - 1].clone()
    return last


class Linearization:
    """``IterativeSolver.linearize``: a solve with its whole trajectory kept, to push any number of directions through."""

    def __init__(self, eng, omega: float, sos, k_sq, src, start, tape, rmse):
        self._eng, self._omega, self._sos, self._k_sq, self._src, self._start, self._tape = eng, omega, sos, k_sq, src, start, tape
        self.wavefield, self.residual, self.rmse = tape[0][-1], tape[1][-1], rmse

    def jvp(self, d_sos=None, d_source=None) -> dict:
        """Tangents of the final wavefield, residual and RMSE along (d_sos [B,1,n,n], d_source shaped like the source); None = zero."""
        from .autograd import rmse_tangent
        d_sos, d_source = _jvp_directions(self._sos, self._src, d_sos, d_source)
        t_k, t_wf, t_res = jvp_initial_tangents(self._omega, self._sos, d_sos, d_source)
        t_st = torch.zeros_like(self._start[2])
        self._eng.step_jvp(*self._start, self._k_sq, self._src.shape[0], *self._tape, t_wf, t_res, t_st, t_k, d_source)
        return {"d_wavefield": t_wf, "d_residual": t_res, "d_rmse": rmse_tangent(t_res, self.residual, self.rmse)}


def _jvp_directions(sos, src, d_sos, d_source):
    if d_sos is not None:
        if tuple(d_sos.shape) != tuple(sos.shape):
            raise ValueError(f"d_sos has shape {tuple(d_sos.shape)}, expected {tuple(sos.shape)}")
        d_sos = d_sos.detach().to(sos.device).float().contiguous()
    if d_source is not None:
        if tuple(d_source.shape) != tuple(src.shape):
            raise ValueError(f"d_source has shape {tuple(d_source.shape)}, expected the source's {tuple(src.shape)}")
        d_source = d_source.detach().to(sos.device).float().contiguous()
    return d_sos, d_source


class IterativeSolver(nn.Module):
    def __init__(
        self,
        domain_size: int,
        k: float,
        omega: float,
        PMLsize: int,
        sigma_max: float,
        source_location: list,
        train_data_path: Optional[str] = None,
        validation_data_path: Optional[str] = None,
        test_data_path: Optional[str] = None,
        activation_function: str = "relu",
        architecture: str = "custom_unet",
        gradient_clip_val: int = 0,
        batch_size: int = 24,
        buffer_size: int = 1000,
        depth: int = 4,
        features: int = 8,
        learning_rate: float = 1e-4,
        loss: str = "mse",
        minimum_learning_rate: float = 1e-4,
        optimizer: str = "adam",
        weight_decay: float = 0.0,
        max_iterations: int = 100,
        source_amplitude: int = 10,
        source_phase: int = 0,
        source_smoothing: bool = False,
        state_channels: int = 2,
        state_depth: int = 4,
        unrolling_steps: int = 10,
    ):
        super().__init__()
        hp = dict(locals())
        hp.pop("self")
        hp.pop("__class__", None)
        self.hparams = AttributeDict(hp)  # save_hyperparameters() equivalent (hybridnet.py:54)
        self._engine: Optional[Engine] = None
        self._differentiable = False   # differentiable(True): the autograd path even when only the parameters require grad
        self._unet_precision = None   # None: the library default (fp32, or HN_UNET_IMPL at context creation)
        self.register_buffer("sigmas", None)
        self.set_laplacian()
        self.setup_source()
        self.init_f()

        def weights_init(m):  # hybridnet.py:70-75 (overwritten by load_state_dict)
            if isinstance(m, nn.Conv2d):
                torch.nn.init.xavier_normal_(m.weight, gain=0.02)

        self.f.apply(weights_init)

    # ------------------------------------------------------------------ construction -----
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict: bool = True, **kwargs):
        """Lightning's classmethod: hyper_parameters (+ overrides) -> cls(**hp) -> load_state_dict."""
        hp, sd = read_lightning_checkpoint(checkpoint_path, map_location or "cpu")
        hp.update(kwargs)
        model = cls(**hp)
        model.load_state_dict(sd, strict=strict)
        return model

    @classmethod
    def from_exported_weights(cls, npz_path: Optional[str] = None, hparams_json: Optional[str] = None, **kwargs):
        """Build from the `f.*` tensors exported out of the shipped checkpoint (package data, helmnet_amd/data)."""
        from .checkpoint import default_exported_weights, read_exported_weights
        d_npz, d_json = default_exported_weights()
        hp, sd = read_exported_weights(npz_path or d_npz, hparams_json or d_json)
        hp.update(kwargs)
        model = cls(**hp)
        model.load_state_dict(sd, strict=False)
        return model

    def init_f(self):
        if self.hparams.architecture != "custom_unet":
            raise NotImplementedError("Unknown architecture {}".format(self.hparams.architecture))
        self.f = HybridNet(
            activation_function=self.hparams.activation_function,
            depth=self.hparams.depth,
            domain_size=self.hparams.domain_size,
            features=self.hparams.features,
            inchannels=6,
            state_channels=self.hparams.state_channels,
            state_depth=self.hparams.state_depth,
        )

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    @property
    def device(self) -> torch.device:
        return self.source.device

    # ------------------------------------------------------------------ engine -----------
    def engine(self) -> Engine:
        """The library context for this solver's device, with domain + weights in sync."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(
                "IterativeSolver is on the CPU: helmnet_amd computes on MI355X only -- call "
                "solver.to('cuda:0') first (the CPU restatement lives in oracle/ for tests)."
            )
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._engine is None or self._engine.device != dev:
            self._engine = Engine(dev)
        rect = self._rect()
        tail = (int(self.hparams.PMLsize), float(self.hparams.sigma_max), float(self.hparams.k))
        key = ((rect,) if rect else (int(self.hparams.domain_size),)) + tail
        if self._engine.domain_key != key:
            if rect:
                self._engine.set_domain_rect(*rect, *tail)
            else:
                self._engine.set_domain(*key)
        if self._unet_precision is not None and self._engine.unet_precision != self._unet_precision:
            self._engine.set_unet_precision(self._unet_precision)
        self.f.bind(self._engine)
        self.Lap.bind(self._engine)
        self.f.sync_weights(self._engine)
        return self._engine

    # ------------------------------------------------------------------ rectangular domains ---------
    def _rect(self):
        """(H, W) when the domain is rectangular (``set_domain_size((H, W))`` with H != W), else None."""
        ds = self.hparams.domain_size
        return (int(ds[0]), int(ds[1])) if isinstance(ds, (tuple, list)) else None

    def _require_square(self, what: str):
        """The one refusal of everything the rectangular path does not cover: the library has no kernels for it on H x W (hn_set_domain_rect)."""
        rect = self._rect()
        if rect:
            raise NotImplementedError(f"{what} is not implemented on a rectangular domain ({rect[0]} x {rect[1]}): the rectangular path covers forward, "
                                      "n_steps, single_step, get_residual, apply_laplacian and solve_to_tolerance without gradients in fp32")

    # ------------------------------------------------------------------ autograd ---------
    def differentiable(self, on: bool = True):
        """Route forward / n_steps / single_step / get_residual / apply_laplacian through autograd (helmnet_amd.autograd) whenever grad mode
        is on, even if no input tensor requires grad: weight gradients for a loss of the caller's own over plain inputs.  Off by default --
        an un-frozen solver's parameters alone do not switch the (taping) autograd path on.  Returns self."""
        self._differentiable = bool(on)
        return self

    def _wants_grad(self, *tensors, states: bool = False) -> bool:
        """The autograd path: grad mode is on and an input tensor (or the source map, or with ``states`` a hidden state held in f) requires
        grad -- or differentiable(True) was called."""
        if not torch.is_grad_enabled():
            return False
        ts = [t for t in tensors if isinstance(t, torch.Tensor)] + [self.source]
        if states:
            ts += [enc.state for enc in self.f.enc if enc.state is not None]
        wanted = self._differentiable or any(t.requires_grad for t in ts)
        if wanted:
            self._require_square("the autograd path")
        return wanted

    def _check_grad_precision(self, eng: Engine):
        if eng.unet_precision not in ("fp32", "valu"):
            raise NotImplementedError(f"gradients through the solver are computed for the fp32 UNet only (this solver runs {eng.unet_precision!r}; "
                                      "call set_unet_precision('fp32'), or run under torch.no_grad())")

    def _src_graph(self) -> torch.Tensor:
        src = self.source.float()
        return src if src.is_contiguous() else src.contiguous()

    def _run_autograd(self, wf, res, k_sq, num_iterations, return_wavefields, return_states, residuals: str, checkpoint_every: int):
        """_run on the autograd path (helmnet_amd.autograd.Solve): same outputs, carrying grad_fn."""
        from .autograd import Solve, SolveSpec, weight_blob
        eng = self.engine()
        self._check_grad_precision(eng)
        K = int(num_iterations)
        st = self.f.get_states(flatten=True).float()
        if K <= 0:
            self.f.adopt_states(st)
            return {"wavefields": [wf], "residuals": [res] if residuals in ("all", "last") else [], "states": [], "last_iteration": K - 1,
                    "residual_norms": None, **({"last_residual": res} if residuals == "norms" else {})}
        want_w = any(p.requires_grad for p in self.f.parameters())
        with torch.set_grad_enabled(want_w):
            blob = weight_blob(self.f)
        stateless = [tuple(bd) for d, bd in enumerate(self.f.state_boundaries) if d >= self.f.state_depth]
        spec = SolveSpec(eng, K, checkpoint_every, bool(return_wavefields), residuals == "all", bool(return_states), stateless)
        wf_o, res_o, st_o, rmse = Solve.apply(spec, wf.float().contiguous(), res.float().contiguous(), st.contiguous(), k_sq.float().contiguous(),
                                              self._src_graph(), blob)
        self.f.adopt_states(st_o[-1])
        out = {
            "wavefields": list(wf_o.unbind(0)),
            "residuals": list(res_o.unbind(0)) if residuals in ("all", "last") else [],
            "states": list(st_o.unbind(0)) if return_states else [],
            "last_iteration": K - 1,
            "residual_norms": rmse,
        }
        if residuals == "norms":
            out["last_residual"] = res_o[-1]
        return out

    def set_unet_precision(self, mode: str):
        """Extension (BASELINE.json configs[4]): arithmetic of the UNet convolutions -- 'fp32' (the reference's,
        default), 'fp16' (mixed fp16 UNet / fp32 spectral residual), 'bf16x3' / 'bf16x2' (split-bf16 emulations),
        'valu'.  Per solver (hn_set_unet_precision on its context), not per process."""
        from . import _lib
        if mode not in _lib.HN_PRECISION:
            raise ValueError(f"unknown UNet precision {mode!r} (choose from {sorted(_lib.HN_PRECISION)})")
        if mode not in ("fp32", "valu"):
            self._require_square(f"the 16-bit UNet precision {mode!r}")
        self._unet_precision = mode
        if self._engine is not None:
            self._engine.set_unet_precision(mode)

    # ------------------------------------------------------------------ setup ------------
    def set_domain_size(self, domain_size, source_location=None, source_map=None):
        """hybridnet.py:92-108.  ``domain_size``: an int as in the reference, or (extension) a pair (H, W) of rows and columns with
        ``source_location=[row, col]`` or ``source_map=[S, 2, H, W]``; a pair with H == W is the int."""
        if isinstance(domain_size, (tuple, list)):
            h, w = domain_hw(domain_size)
            domain_size = h if h == w else (h, w)
            if h != w and self._unet_precision not in (None, "fp32", "valu"):
                raise NotImplementedError(f"the 16-bit UNet precision {self._unet_precision!r} is not implemented on a rectangular domain ({h} x {w})")
        self.hparams.domain_size = domain_size
        self.f.domain_size = self.hparams.domain_size
        self.set_laplacian()
        # the reference builds the source module at hparams.source_location first and only then
        # moves it (hybridnet.py:96,101-104), which indexes out of bounds when the checkpoint's
        # location does not fit the new domain; build it at the requested location directly.
        self.setup_source(location=source_location)
        self.Lap.to(self.device)
        self.source_module.to(self.device)
        if source_location is not None:
            self.set_multiple_sources([source_location])
        else:
            self.set_source_maps(source_map)
        self.f.init_by_size()
        for enc, size in zip(self.f.enc, self.f.states_dimension):
            enc.domain_size = size
            enc.state = None

    def set_laplacian(self):
        dev = self.source.device if hasattr(self, "source") else torch.device("cpu")
        self.Lap = FastLaplacianWithPML(
            domain_size=self.hparams.domain_size,
            PMLsize=self.hparams.PMLsize,
            k=self.hparams.k,
            sigma_max=self.hparams.sigma_max,
        )
        sx, sy = self.Lap.sigmas()
        self.sigmas = torch.stack([sx.detach().clone(), sy.detach().clone()]).float().to(dev)

    def setup_source(self, location=None):
        n = self.hparams.domain_size
        if location is None:
            h, w = domain_hw(n)
            location = self.hparams.source_location
            if not (0 <= location[0] < h and 0 <= location[1] < w):
                location = [h // 2, w // 2]  # placeholder; a source map / location is set right after
        self.source_module = SourceModule(
            image_size=n,
            omega=self.hparams.omega,
            location=location,
            amplitude=self.hparams.source_amplitude,
            phase=self.hparams.source_phase,
            smooth=self.hparams.source_smoothing,
        )
        with torch.no_grad():
            self.set_source()

    def set_source_maps(self, sourceval):
        dev = self.source.device if hasattr(self, "source") else sourceval.device
        self.source = nn.Parameter(sourceval.to(dev), requires_grad=False)

    def set_source(self):
        self.set_source_maps(self.source_module.spatial_map(0).permute(0, 3, 1, 2).contiguous())

    def reset_source(self):
        with torch.no_grad():
            if not self.source_module.get_location() == self.hparams.source_location:
                self.source_module.set_new_location(self.hparams.source_location)
                self.set_source()

    def set_multiple_sources(self, source_locations):
        maps = []
        with torch.no_grad():
            for loc in source_locations:
                self.source_module.set_new_location(loc)
                maps.append(self.source_module.spatial_map(0).permute(0, 3, 1, 2))
            self.set_source_maps(torch.cat(maps, 0).contiguous())

    # ------------------------------------------------------------------ operators --------
    @staticmethod
    def test_loss_function(x):
        """Per-sample residual RMSE (hybridnet.py:295-297); plain tensor reduction for callers
        that hold a residual tensor -- the solver loop itself uses the fused hn_step norms."""
        return x.pow(2).mean((1, 2, 3)).sqrt()

    def loss_function(self, x):
        """hybridnet.py:285-293: mean square over every element ('mse' is the only loss the reference implements)."""
        if self.hparams.loss == "mse":
            return x.pow(2).mean()
        raise NotImplementedError("The loss function {} is not implemented".format(self.hparams.loss))

    def get_random_source_loc(self):
        """hybridnet.py:178-190: a random source location on a circle of radius L - PMLsize - 2 around the domain centre."""
        import numpy as np
        self._require_square("get_random_source_loc")
        theta = 2 * np.pi * np.random.rand()
        L = self.hparams.domain_size // 2
        dL = L - self.hparams.PMLsize - 2
        return [int(L + dL * np.cos(theta)), int(L + dL * np.sin(theta))]

    def validation_step(self, batch, batch_idx=0):
        """hybridnet.py:333-352: one random source per sample, max_iterations solver iterations, loss = sqrt(mean(res_last^2)) over the
        batch (NaN -> inf); returns the loss, the first sample's wavefield mapped to [0, 1] and the batch index."""
        self.set_multiple_sources([self.get_random_source_loc() for _ in range(batch.shape[0])])
        output = self.forward(batch, num_iterations=self.hparams.max_iterations, return_wavefields=False, return_states=False, residuals="last")
        loss = self.loss_function(output["residuals"][-1]).sqrt()
        loss = torch.where(torch.isnan(loss), torch.full_like(loss, float("inf")), loss)
        sample_wavefield = (torch.nn.functional.hardtanh(output["wavefields"][0][0]) + 1) / 2
        return {"loss": loss, "sample_wavefield": sample_wavefield, "batch_idx": batch_idx}

    def test_step(self, batch, batch_idx=0):
        """hybridnet.py:299-314: max_iterations iterations with every wavefield kept; per-sample residual RMSE after every iteration
        ([B, max_iterations], from the fused on-device norms) and the list of wavefields."""
        self.reset_source()
        output = self.forward(batch, num_iterations=self.hparams.max_iterations, return_wavefields=True, return_states=False, residuals="norms")
        return {"losses": output["residual_norms"].transpose(0, 1).contiguous(), "wavefields": list(output["wavefields"])}

    def trainer(self, **kwargs):
        """The training half of the reference class (replay buffer, training_step, Adam + ReduceLROnPlateau) for this solver."""
        from .training import Trainer
        self._require_square("trainer()")
        return Trainer(self, **kwargs)

    def get_initials(self, sos_maps: torch.Tensor):
        k_sq = (self.hparams.omega / sos_maps) ** 2
        wavefield = torch.zeros(k_sq.shape[0], 2, k_sq.shape[2], k_sq.shape[3], device=k_sq.device)
        return k_sq, wavefield

    def _src(self) -> torch.Tensor:
        return self.source.detach().float().contiguous()

    def apply_laplacian(self, x: torch.Tensor):
        if self._wants_grad(x):
            from .autograd import Laplacian
            return Laplacian.apply(self.engine(), x.float())
        return self.engine().laplacian(x.float().contiguous())

    def _refuse_medium_grad(self, what: str, density: bool, *tensors):
        """Absorbing media and variable density have one differentiable path, the adjoint-state gradients of ``solve_implicit`` (which detaches
        before it comes here); the library has no derivative of either solver LOOP: an input that requires grad -- or
        differentiable(True) under grad mode -- raises before anything touches the device.  ``density``: the medium has one, and is named for it."""
        if any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors) or (self._differentiable and torch.is_grad_enabled()):
            name, operator = ("density", "variable-density") if density else ("absorption", "lossy")
            raise RuntimeError(f"{what} with {name} runs without gradients (the library has no derivative of the {operator} operator): pass detached "
                               "tensors, or run under torch.no_grad() after differentiable(True)")

    @staticmethod
    def _rho_grad(density, like: torch.Tensor) -> torch.Tensor:
        """``rho_grad`` [B,2,H,W] fp32 of a ``density`` broadcastable to ``like`` [B,1,H,W]: helmnet_amd.density.log_density_gradient."""
        from .density import log_density_gradient
        if not isinstance(density, torch.Tensor):
            raise TypeError("density must be a tensor broadcastable to the sound-speed maps")
        rho = density.detach().to(like.device, torch.float32)
        try:
            rho = rho.expand_as(like)
        except RuntimeError as e:
            raise ValueError(f"density of shape {tuple(density.shape)} does not broadcast to {tuple(like.shape)}") from e
        return log_density_gradient(rho.contiguous())

    def _initials(self, what: str, sos_maps, absorption=None, density=None):
        """(Medium, wf = 0) of a solve without gradients on (sos_maps, absorption or None, density or None): ``get_initials`` for the lossless medium
        of constant density, else helmnet_amd.absorption.complex_k_sq and ``_rho_grad``."""
        sos = sos_maps.float().contiguous()
        if absorption is None and density is None:
            k_sq, wf = self.get_initials(sos)
            return Medium(k_sq.contiguous()), wf
        self._refuse_medium_grad(what, density is not None, sos_maps, absorption, density)
        if absorption is not None:
            from .absorption import complex_k_sq
            if isinstance(absorption, torch.Tensor):
                absorption = absorption.detach().to(sos.device, sos.dtype)
            k_sq, k_sq_im = complex_k_sq(sos, absorption, self.hparams.omega)
        else:
            k_sq, k_sq_im = self.get_initials(sos)[0].contiguous(), None
        rho_grad = None if density is None else self._rho_grad(density, k_sq)
        return Medium(k_sq, k_sq_im, rho_grad), torch.zeros(sos.shape[0], 2, sos.shape[2], sos.shape[3], device=sos.device)

    def get_residual(self, x: torch.Tensor, k_sq: torch.Tensor, k_sq_im: Optional[torch.Tensor] = None, rho_grad: Optional[torch.Tensor] = None):
        """hybridnet.py:544-556.  ``k_sq_im`` (extension, [B,1,H,W]): the imaginary plane of an absorbing medium's squared wavenumber
        (helmnet_amd.absorption.complex_k_sq); the residual is then L(x) + (k_sq + i k_sq_im) x - source, without gradients.
        ``rho_grad`` (extension, [B,2,H,W]): the gradient of ln rho (helmnet_amd.density.log_density_gradient); the residual is then the
        variable-density operator's (hn_residual_medium), with or without ``k_sq_im``, without gradients."""
        if k_sq_im is not None or rho_grad is not None:
            self._refuse_medium_grad("get_residual", rho_grad is not None, x, k_sq, k_sq_im, rho_grad)
            m = Medium(*(None if t is None else t.float().contiguous() for t in (k_sq, k_sq_im, rho_grad)))
            return getattr(self.engine(), "residual" + m.kind)(x.float().contiguous(), *m.planes(), self._src())
        if self._wants_grad(x, k_sq):
            from .autograd import Residual
            return Residual.apply(self.engine(), x.float(), k_sq.float(), self._src_graph())
        return self.engine().residual(x.float().contiguous(), k_sq.float().contiguous(), self._src())

    def get_residual64(self, wavefield: torch.Tensor, k_sq: torch.Tensor, k_sq_im: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The residual of ``get_residual`` evaluated in float64 on the GPU (the reference's ``solver.double().get_residual``), [B,2,n,n] float64.
        fp32 inputs are up-cast exactly: the problem checked is the one with the fp32 ``k_sq`` and source the solver ran.  No gradients.
        ``k_sq_im`` (extension, [B,1,H,W]): the lossy float64 residual L(x) + (k_sq + i k_sq_im) x - source (hn_residual_f64_lossy), on square and
        rectangular domains; None: the code path and the bits of before."""
        if k_sq_im is not None:
            return self._residual64_lossy(wavefield, k_sq, k_sq_im, True, False)[0]
        return self._residual64(wavefield, k_sq, True, False)[0]

    def _residual64_lossy(self, wavefield, k_sq, k_sq_im, want_res: bool, want_rmse: bool):
        _require_no_grad("the float64 residual check", wavefield, k_sq, k_sq_im)
        return self.engine().residual64_lossy(wavefield.double().contiguous(), k_sq.double().contiguous(), k_sq_im.double().contiguous(),
                                              self.source.detach().double().contiguous(), want_res, want_rmse)

    def _residual64(self, wavefield, k_sq, want_res: bool, want_rmse: bool):
        _require_no_grad("the float64 residual check", wavefield, k_sq)
        self._require_square("the float64 residual check")
        return self.engine().residual64(wavefield.double().contiguous(), k_sq.double().contiguous(), self.source.detach().double().contiguous(),
                                        want_res, want_rmse)

    def verify(self, wavefield: torch.Tensor, sos_maps: Optional[torch.Tensor] = None, k_sq: Optional[torch.Tensor] = None, absorption=None,
               k_sq_im: Optional[torch.Tensor] = None) -> dict:
        """How far the fp32 residual norm of ``wavefield`` can be trusted.  Pass exactly one of ``sos_maps`` / ``k_sq`` (the fp32 problem the solver ran).
        Returns per sample: ``residual_norm64`` (float64 RMSE of the float64 residual), ``residual_norm32`` (what hn_residual + hn_rmse give) and
        ``evaluator_error`` = RMSE of (fp32 residual - float64 residual), the floor below which an fp32 residual norm carries no information.
        Absorbing media: ``absorption`` (alpha, as in ``forward``) goes with ``sos_maps``, ``k_sq_im`` with ``k_sq``; any other pairing raises
        ValueError.  The same three keys come from hn_residual_lossy and hn_residual_f64_lossy, on square and rectangular domains.  With both None:
        the code path and the bits of before."""
        if absorption is not None or k_sq_im is not None:
            return self._verify_lossy(wavefield, sos_maps, k_sq, absorption, k_sq_im)
        self._require_square("verify")
        if (sos_maps is None) == (k_sq is None):
            raise ValueError("pass exactly one of sos_maps and k_sq")
        _require_no_grad("verify", wavefield, sos_maps, k_sq)
        if k_sq is None:
            k_sq = self.get_initials(sos_maps.float().contiguous())[0]
        eng = self.engine()
        wf32, k32 = wavefield.float().contiguous(), k_sq.float().contiguous()
        res32 = eng.residual(wf32, k32, self._src())
        res64, norm64 = self._residual64(wavefield, k32, True, True)
        diff = res32.double() - res64
        return {"residual_norm64": norm64, "residual_norm32": eng.rmse(res32), "evaluator_error": diff.pow(2).mean((1, 2, 3)).sqrt()}

    def _verify_lossy(self, wavefield, sos_maps, k_sq, absorption, k_sq_im) -> dict:
        if (sos_maps is None) == (k_sq is None):
            raise ValueError("pass exactly one of sos_maps and k_sq")
        if absorption is not None and k_sq_im is not None:
            raise ValueError("pass one of absorption (with sos_maps) and k_sq_im (with k_sq), not both")
        if absorption is not None and sos_maps is None:
            raise ValueError("absorption goes with sos_maps (with k_sq pass k_sq_im)")
        if k_sq_im is not None and k_sq is None:
            raise ValueError("k_sq_im goes with k_sq (with sos_maps pass absorption)")
        self._refuse_medium_grad("verify", False, wavefield, sos_maps, k_sq, absorption, k_sq_im)
        if k_sq is None:
            k_sq, k_sq_im, _ = self._initials("verify", sos_maps, absorption)[0]
        eng = self.engine()
        wf32, k32, ki32 = wavefield.float().contiguous(), k_sq.float().contiguous(), k_sq_im.float().contiguous()
        res32 = eng.residual_lossy(wf32, k32, ki32, self._src())
        res64, norm64 = self._residual64_lossy(wavefield, k32, ki32, True, True)
        diff = res32.double() - res64
        return {"residual_norm64": norm64, "residual_norm32": eng.rmse(res32), "evaluator_error": diff.pow(2).mean((1, 2, 3)).sqrt()}

    def single_step(self, wavefield, k_sq, residual, get_residual: bool = True):
        """One iteration on caller-held tensors (hybridnet.py:558-584); network states live in
        ``self.f`` as in the reference.  Inputs are not modified.  With an input (or a state held in f, or the source) requiring
        grad the step is differentiable and the new states stored in f carry their grad_fn, so chained calls back-propagate through
        the hidden states as in the reference."""
        eng = self.engine()
        if any(enc.state is None for enc in self.f.enc):
            raise ValueError("You must set or clear the state before using this module")
        if self._wants_grad(wavefield, k_sq, residual, states=True):
            out = self._run_autograd(wavefield, residual, k_sq, 1, False, False, "last", 1)
            wf, res = out["wavefields"][0], out["residuals"][0]
            return (wf, res) if get_residual else wf
        wf = wavefield.detach().float().clone().contiguous()
        res = residual.detach().float().clone().contiguous()
        st = self.f.get_states(flatten=True).float().contiguous().clone()
        keep = self.f.to_engine_states(st)
        eng.step(wf, res, st, k_sq.float().contiguous(), self._src(), 1)
        self.f.from_engine_states(keep, st)
        self.f.adopt_states(st)
        return (wf, res) if get_residual else wf

    # ------------------------------------------------------------------ loops ------------
    def _loop(self, wf, res, st, m: Medium, src, num_iterations, return_wavefields, return_states, residuals: str):
        """K iterations on wf / res / st, updated in place -- Engine.step64 for float64 tensors, else Engine.step, step_lossy or step_medium by the
        kind of the medium ``m`` -- with the histories asked for, in wf's dtype; the result dictionary of ``forward``."""
        eng = self.engine()
        b, hw, K = wf.shape[0], tuple(wf.shape[-2:]), int(num_iterations)

        def hist(shape, what):
            try:
                return torch.empty(shape, device=wf.device, dtype=wf.dtype)
            except RuntimeError as e:  # out of memory
                raise RuntimeError(
                    f"cannot keep {what} for {K} iterations ({shape}); pass residuals='norms' or 'last' "
                    "to IterativeSolver.forward, or fewer iterations"
                ) from e

        res_hist = hist((K, b, 2) + hw, "every residual") if residuals == "all" and K > 0 else None
        wf_hist = hist((K, b, 2) + hw, "every wavefield") if return_wavefields and K > 0 else None
        st_hist = hist((K, b, 2, eng.state_len), "every hidden state") if return_states and K > 0 else None
        rmse = torch.empty((K, b), device=wf.device, dtype=wf.dtype) if K > 0 else None
        if K > 0:
            keep = self.f.to_engine_states(st)      # levels without state: zeros in, the caller's values back out
            step = eng.step64 if wf.dtype == torch.float64 else getattr(eng, "step" + m.kind)
            step(wf, res, st, *m.planes(), src, K, res_hist, wf_hist, st_hist, rmse)
            self.f.from_engine_states(keep, st, st_hist)
        out = {
            "wavefields": list(wf_hist.unbind(0)) if wf_hist is not None else [wf],
            "residuals": list(res_hist.unbind(0)) if res_hist is not None else ([res] if residuals == "last" else []),
            "states": list(st_hist.unbind(0)) if st_hist is not None else [],
            "last_iteration": K - 1,
            "residual_norms": rmse,  # [K, B] per-sample RMSE (extension; the reference derives it afterwards)
        }
        if residuals == "norms":
            out["last_residual"] = res
        return out

    def _run(self, wf, res, st, m: Medium, num_iterations, return_wavefields, return_states, residuals: str):
        out = self._loop(wf, res, st, m, self._src(), num_iterations, return_wavefields, return_states, residuals)
        self.f.adopt_states(st)
        return out

    def forward(self, sos_maps, return_wavefields=False, return_states=False, num_iterations=None,
                stop_if_diverge=False, residuals: str = "all", checkpoint_every: int = 1, absorption=None, density=None):
        """hybridnet.py:654-697.  ``residuals``: "all" keeps every residual tensor like the
        reference (K x B x 2 x N x N floats), "norms" keeps only the per-iteration per-sample RMSE
        (``out["residual_norms"]``), "last" only the final residual.

        Differentiable (helmnet_amd.autograd) when grad mode is on and ``sos_maps``, the source map or a hidden state requires grad, or
        after ``differentiable(True)``; weight gradients then reach f's parameters if they require grad.  The autograd path keeps the
        wavefield / residual / state of every iteration as its tape -- with residuals="norms" too -- or, with ``checkpoint_every`` = c > 1,
        those of every c-th iteration only: backward re-runs the segments in between (same gradients, bit for bit).  Without
        gradients ``checkpoint_every`` is ignored.

        ``absorption`` (extension; None: the code path and the bits of before): alpha in nepers per grid point, a number or a tensor broadcastable
        to ``sos_maps`` -- the medium is k~ = omega / sos + i alpha (helmnet_amd.absorption) and the loop runs on ``hn_step_lossy``.  Same keys and
        shapes; no gradients: an input that requires grad raises RuntimeError.

        ``density`` (extension; None: the code path and the bits of before): rho, a tensor broadcastable to ``sos_maps`` -- only its ratios matter,
        and a map with jumps should be smoothed first (helmnet_amd.density).  The loop runs on ``hn_step_medium``, with or without ``absorption``;
        no gradients, as with ``absorption``."""
        if residuals not in ("all", "norms", "last"):
            raise ValueError("residuals must be 'all', 'norms' or 'last'")
        if num_iterations is None:
            num_iterations = self.hparams.max_iterations
        if absorption is None and density is None and self._wants_grad(sos_maps):
            k_sq, wf = self.get_initials(sos_maps.float())
            self.f.clear_states(wf)
            res = self.get_residual(wf, k_sq)
            return self._run_autograd(wf, res, k_sq, num_iterations, return_wavefields, return_states, residuals, checkpoint_every)
        m, wf = self._initials("forward", sos_maps, absorption, density)
        self.f.clear_states(wf)
        res = self.get_residual(wf, *m)
        st = self.f.get_states(flatten=True).contiguous()
        return self._run(wf, res, st, m, num_iterations, return_wavefields, return_states, residuals)

    def n_steps(self, wavefield, k_sq, residual, num_iterations, return_wavefields=False, return_states=False,
                residuals: str = "all", checkpoint_every: int = 1, absorption=None, density=None):
        """hybridnet.py:586-623: continue from given wavefield / residual and the states held in f.  Differentiable as ``forward``
        when an input, a state held in f or the source requires grad (``checkpoint_every``: see ``forward``).

        ``absorption`` (extension; None: the code path and the bits of before): alpha, as in ``forward``.  ``k_sq`` is then the REAL plane of the
        medium, (omega / sos)^2 - alpha^2 as ``complex_k_sq`` returns it, and the imaginary plane is formed from the two:
        2 sqrt(k_sq + alpha^2) alpha.  No gradients.

        ``density`` (extension; None: the code path and the bits of before): rho, as in ``forward``, broadcastable to ``k_sq``.  No gradients."""
        if absorption is not None or density is not None:
            self._refuse_medium_grad("n_steps", density is not None, wavefield, k_sq, residual, absorption, density)
        elif self._wants_grad(wavefield, k_sq, residual, states=True):
            return self._run_autograd(wavefield, residual, k_sq, num_iterations, return_wavefields, return_states, residuals, checkpoint_every)
        kq, k_sq_im = k_sq.float().contiguous(), None
        if absorption is not None:
            alpha = torch.as_tensor(absorption, dtype=kq.dtype, device=kq.device).expand_as(kq)
            k_sq_im = (2.0 * (kq + alpha * alpha).sqrt() * alpha).contiguous()
        m = Medium(kq, k_sq_im, None if density is None else self._rho_grad(density, kq))
        return self._n_steps_no_grad(wavefield, m, residual, num_iterations, return_wavefields, return_states, residuals)

    def _n_steps_no_grad(self, wavefield, m: Medium, residual, num_iterations, return_wavefields=False, return_states=False, residuals: str = "all"):
        """``n_steps`` without gradients on the medium ``m``: the inputs are not modified."""
        wf = wavefield.detach().float().clone().contiguous()
        res = residual.detach().float().clone().contiguous()
        st = self.f.get_states(flatten=True).float().contiguous().clone()
        return self._run(wf, res, st, m, num_iterations, return_wavefields, return_states, residuals)

    # ------------------------------------------------------------------ forward mode ----
    def _jvp_setup(self, sos_maps):
        """(engine, sos, k_sq, source, wf0 = 0, res0, zero flat states) of a solve from cleared states; the states held in f are not touched."""
        self._require_square("the forward-AD path (jvp / linearize)")
        eng = self.engine()
        self._check_grad_precision(eng)
        sos = sos_maps.detach().to(self.device).float().contiguous()
        k_sq, wf = self.get_initials(sos)
        k_sq, src = k_sq.contiguous(), self._src()
        res = eng.residual(wf, k_sq, src)
        st = torch.zeros(sos.shape[0], 2, eng.state_len, device=sos.device, dtype=torch.float32)
        return eng, sos, k_sq, src, wf, res, st

    def jvp(self, sos_maps, d_sos=None, d_source=None, num_iterations=None, chunk: int = 25) -> dict:
        """Extension: the solve of ``forward`` together with its directional derivative along (``d_sos`` [B,1,n,n], ``d_source`` shaped like
        the source map; None = zero), in forward mode (hn_step_jvp).  Primal and tangent run interleaved, ``chunk`` iterations at a time, so
        memory is O(chunk) whatever the iteration count.  Returns wavefield, residual, rmse [B] and d_wavefield, d_residual, d_rmse.  The
        weights are constants; several directions at once: repeat the batch.  The hidden states held in ``f`` are neither read nor written."""
        from .autograd import rmse_tangent
        _require_no_grad("jvp", sos_maps, d_sos, d_source)
        K = int(self.hparams.max_iterations if num_iterations is None else num_iterations)
        if K < 1 or int(chunk) < 1:
            raise ValueError("jvp needs num_iterations >= 1 and chunk >= 1")
        eng, sos, k_sq, src, wf, res, st = self._jvp_setup(sos_maps)
        d_sos, d_source = _jvp_directions(sos, src, d_sos, d_source)
        t_k, t_wf, t_res = jvp_initial_tangents(float(self.hparams.omega), sos, d_sos, d_source)
        t_st = torch.zeros_like(st)
        rmse = jvp_chunks(eng, wf, res, st, k_sq, src, t_wf, t_res, t_st, t_k, d_source, K, chunk)
        return {"wavefield": wf, "residual": res, "rmse": rmse, "d_wavefield": t_wf, "d_residual": t_res, "d_rmse": rmse_tangent(t_res, res, rmse)}

    def linearize(self, sos_maps, num_iterations=None) -> Linearization:
        """Extension: solve once keeping the whole trajectory (O(num_iterations) memory) and return an object with ``.wavefield``,
        ``.residual`` and ``.jvp(d_sos=None, d_source=None)``, callable repeatedly: one column of the Jacobian per call."""
        _require_no_grad("linearize", sos_maps)
        K = int(self.hparams.max_iterations if num_iterations is None else num_iterations)
        if K < 1:
            raise ValueError("linearize needs num_iterations >= 1")
        eng, sos, k_sq, src, wf, res, st = self._jvp_setup(sos_maps)
        start = (wf.clone(), res.clone(), st.clone())
        new = lambda *shape: torch.empty(shape, device=sos.device, dtype=torch.float32)  # noqa: E731
        tape = (new(K, *wf.shape), new(K, *res.shape), new(K, *st.shape))
        rmse = new(K, sos.shape[0])
        eng.step(wf, res, st, k_sq, src, K, tape[1], tape[0], tape[2], rmse)
        return Linearization(eng, float(self.hparams.omega), sos, k_sq, src, start, tape, rmse[K - 1])

    # ------------------------------------------------------------------ the loop in float64 ----
    def _source64(self, source, batch: int) -> torch.Tensor:
        self._require_square("the float64 loop (forward64 / n_steps64 / deviation_from_float64)")
        n = int(self.hparams.domain_size)
        if source is None:
            return self.source.detach().double().contiguous()
        if source.dtype != torch.float64 or source.dim() != 4 or tuple(source.shape[1:]) != (2, n, n) or source.shape[0] not in (1, batch):
            raise ValueError(f"source must be a float64 [1 or {batch}, 2, {n}, {n}] tensor, got {source.dtype} {tuple(source.shape)}")
        return source.detach().to(self.device).contiguous()

    def _run64(self, wf, res, st, k_sq, src, num_iterations, return_wavefields, return_states, residuals: str):
        """``_run`` on hn_step_f64: wf / res / st (float64, owned by the caller of this helper) are updated in place; nothing held in f is touched."""
        if residuals not in ("all", "norms", "last"):
            raise ValueError("residuals must be 'all', 'norms' or 'last'")
        return self._loop(wf, res, st, Medium(k_sq), src, num_iterations, return_wavefields, return_states, residuals)

    def _initials64(self, sos_maps, source):
        """(wf = 0, residual, zero flat states, k_sq, source), all float64: get_initials on a float64 input (hybridnet.py:522-538) and cleared states."""
        self._require_square("the float64 loop (forward64 / n_steps64 / deviation_from_float64)")
        eng = self.engine()
        sos = sos_maps.detach().to(self.device).double().contiguous()
        src = self._source64(source, sos.shape[0])
        k_sq = ((self.hparams.omega / sos) ** 2).contiguous()
        wf = torch.zeros(sos.shape[0], 2, sos.shape[2], sos.shape[3], device=sos.device, dtype=torch.float64)
        st = torch.zeros(sos.shape[0], 2, eng.state_len, device=sos.device, dtype=torch.float64)
        return wf, eng.residual64(wf, k_sq, src, True, False)[0], st, k_sq, src

    def forward64(self, sos_maps, num_iterations=None, return_wavefields=False, return_states=False, residuals: str = "all", source=None):
        """``forward`` with the whole iteration in float64 on the GPU (hn_step_f64): the reference's ``solver.double()`` run, the trajectory the fp32 /
        fp16 / bf16 modes are measured against.  Same keys as ``forward``, float64 tensors.  The weights are the solver's fp32 parameters up-cast;
        ``source`` None uses ``self.source.double()``, a float64 [1 or B,2,n,n] map overrides it (a source map BUILT in float64 differs from the
        up-cast fp32 one by ~1e-6).  No gradients; the (fp32) hidden states held in ``f`` are neither read nor written.  A reference, not a fast path."""
        _require_no_grad("forward64", sos_maps, source)
        if num_iterations is None:
            num_iterations = self.hparams.max_iterations
        wf, res, st, k_sq, src = self._initials64(sos_maps, source)
        return self._run64(wf, res, st, k_sq, src, num_iterations, return_wavefields, return_states, residuals)

    def n_steps64(self, wavefield, k_sq, residual, states, num_iterations, return_wavefields=False, return_states=False,
                  residuals: str = "all", source=None):
        """``n_steps`` in float64, continuing from given tensors; the hidden states are passed in (flat [B,2,L]) instead of living in ``f`` and come back
        as ``out["final_states"]``.  Inputs are up-cast if need be and not modified."""
        _require_no_grad("n_steps64", wavefield, k_sq, residual, states, source)
        self._require_square("the float64 loop (forward64 / n_steps64 / deviation_from_float64)")
        self.engine()
        wf, res, st, kq = (t.detach().to(self.device).double().clone().contiguous() for t in (wavefield, residual, states, k_sq))
        out = self._run64(wf, res, st, kq, self._source64(source, wf.shape[0]), num_iterations, return_wavefields, return_states, residuals)
        out["final_states"] = st
        return out

    def deviation_from_float64(self, sos_maps, num_iterations: int, checkpoints) -> dict:
        """How far this solver's current precision mode is from the float64 trajectory on the caller's own maps: ``forward`` and ``forward64`` side by
        side, compared at every iteration count in ``checkpoints``.  Returns ``iterations`` (the sorted checkpoints), ``linf`` [len(checkpoints), B]
        (per-sample max |wavefield - float64 wavefield|), and the residual-norm traces ``rmse32`` / ``rmse64`` [num_iterations, B]."""
        _require_no_grad("deviation_from_float64", sos_maps)
        self._require_square("deviation_from_float64")
        cps = sorted({int(c) for c in checkpoints} | {int(num_iterations)})
        if cps[0] < 1 or cps[-1] > int(num_iterations):
            raise ValueError(f"checkpoints must lie in [1, {int(num_iterations)}]")
        with torch.no_grad():
            wf64, res64, st64, k64, _ = self._initials64(sos_maps, None)
            rows, r32, r64, done = {}, [], [], 0
            for cp in cps:
                if done == 0:
                    o32 = self.forward(sos_maps, num_iterations=cp, residuals="norms")
                    k32 = self.get_initials(sos_maps.float().contiguous())[0].contiguous()
                else:
                    o32 = self.n_steps(o32["wavefields"][0], k32, o32["last_residual"], cp - done, residuals="norms")
                o64 = self.n_steps64(wf64, k64, res64, st64, cp - done, residuals="norms")
                wf64, res64, st64, done = o64["wavefields"][0], o64["last_residual"], o64["final_states"], cp
                r32.append(o32["residual_norms"])
                r64.append(o64["residual_norms"])
                rows[cp] = (o32["wavefields"][0].double() - wf64).abs().amax((1, 2, 3))
        want = sorted({int(c) for c in checkpoints})
        return {"iterations": torch.tensor(want), "linf": torch.stack([rows[c] for c in want]), "rmse32": torch.cat(r32), "rmse64": torch.cat(r64)}

    def solve_to_tolerance(self, sos_maps, tol: float, max_iterations: int = None, check_every: int = 50,
                           norm_reduce=None, verify: bool = False, absorption=None, density=None) -> dict:
        """Extension (BASELINE.json configs[4], "convergence-to-tolerance"): iterate in chunks of
        ``check_every`` until the WORST per-sample residual RMSE (hybridnet.py:295-297) is below ``tol`` or
        ``max_iterations`` is reached.  One device-to-host read of a single float per chunk; with
        ``norm_reduce`` (e.g. helmnet_amd.distributed.allreduce_residual_norms) the test is global over ranks.
        Returns wavefield, last residual, per-iteration RMSE trace [K, B], iterations run and whether it converged.  ``verify=True`` adds the keys of
        ``verify()`` for the final wavefield and ``converged64``: the worst float64 residual norm is below ``tol``.
        ``absorption``: alpha, as in ``forward`` (None: the code path and the bits of before); together with ``verify=True`` it raises
        NotImplementedError: check the returned wavefield with ``verify(wavefield, sos_maps, absorption=...)``.
        ``density``: rho, as in ``forward`` (None: the code path and the bits of before); together with ``verify=True`` it raises
        NotImplementedError (the variable-density operator has no float64 counterpart)."""
        if max_iterations is None:
            max_iterations = self.hparams.max_iterations
        if verify and density is not None:
            raise NotImplementedError("solve_to_tolerance(verify=True) is not implemented with density: the variable-density operator has no float64 "
                                      "residual")
        if verify and absorption is not None:
            raise NotImplementedError("solve_to_tolerance(verify=True) is not implemented with absorption: call verify(wavefield, sos_maps, "
                                      "absorption=...) on the result")
        if verify:
            self._require_square("solve_to_tolerance(verify=True)")
        m, wf = self._initials("solve_to_tolerance", sos_maps, absorption, density)
        k_sq = m.k_sq
        self.f.clear_states(wf)
        res = self.get_residual(wf, *m)
        done, traces, converged = 0, [], False
        while done < max_iterations:
            chunk = min(int(check_every), max_iterations - done)
            if m.kind:
                out = self._n_steps_no_grad(wf, m, res, chunk, residuals="norms")
            else:   # (differentiable where n_steps is)
                out = self.n_steps(wf, k_sq, res, chunk, residuals="norms")
            wf, res = out["wavefields"][0], out["last_residual"]
            traces.append(out["residual_norms"])
            done += chunk
            worst = out["residual_norms"][-1].max() if norm_reduce is None else norm_reduce(out["residual_norms"][-1], "max")
            if float(worst) < tol:
                converged = True
                break
        out = {"wavefield": wf, "residual": res, "residual_norms": torch.cat(traces, 0), "iterations": done, "converged": converged}
        if verify:
            out.update(self.verify(wf, k_sq=k_sq))
            worst64 = out["residual_norm64"].max() if norm_reduce is None else norm_reduce(out["residual_norm64"], "max")
            out["converged64"] = bool(float(worst64) < tol)
        return out

    def gmres(self, sos_maps, restart: int = 20, max_cycles: int = 50, tol: float = 1e-4, x0=None, precondition=None, precond_iterations: int = 10,
              precond_scale=None, absorption=None, density=None) -> dict:
        """The reference's classical baseline (matlab/spectral_gmres_solver.m:86-115) on this solver's operator and source: restarted GMRES with the
        restart cycle fused on the device (``helmnet_amd.gmres.gmres(backend="hip")``), every map stopping on its own.  ``x0`` [B,2,n,n]: the
        starting iterate, e.g. a learned solve's wavefield to be continued by Krylov iterations (default: zeros).  ``precondition="learned"``:
        flexible GMRES with this solver's network as right preconditioner, ``precond_iterations`` iterations per inner step on a right-hand side
        scaled by ``precond_scale`` (None: the source's RMS 2-norm); see ``helmnet_amd.gmres.gmres``.  No gradients.
        ``absorption``: alpha, as in ``forward`` -- the cycles then run on the lossy operator (hn_fgmres_cycle_lossy), preconditioned by the lossy
        learned iteration with ``precondition="learned"``; None: the code path and the bits of before.
        ``density``: rho, as in ``forward`` -- the cycles then run on the variable-density operator (hn_fgmres_cycle_medium), with or without
        ``absorption``; None: the code path and the bits of before."""
        from .gmres import gmres
        self._require_square("gmres")
        medium = {} if density is None else {"density": density}
        return gmres(self, sos_maps, restart=restart, max_outer=max_cycles, tol=tol, x0=x0, backend="hip", precondition=precondition,
                     precond_iterations=precond_iterations, precond_scale=precond_scale, absorption=absorption, **medium)

    def gmres64(self, sos_maps, restart: int = 20, max_cycles: int = 400, tol: float = 1e-10, x0=None, precondition=None, precond_iterations: int = 10,
                precond_scale=None, absorption=None) -> dict:
        """GMRES to float64 accuracy on this solver's operator and source (the role MATLAB's double-precision ``gmres`` has in the reference,
        matlab/spectral_gmres_solver.m:86-115: the ground truth the learned solver is measured against): iterative refinement with the fused fp32
        restart cycle inside and the residual and the update in float64 (``helmnet_amd.gmres.gmres(backend="hip", refine=True)``).  ``tol`` is the
        float64 residual RMSE to reach; ``x0`` [B,2,n,n], fp32 or float64: the starting iterate, e.g. the learned solver's wavefield to be polished
        (default: zeros; it is not written).  Returns ``wavefield`` and ``residual_norms`` in float64.  ``precondition``, ``precond_iterations``,
        ``precond_scale``: as ``gmres`` (the flexible cycle inside the refinement).  No gradients.
        ``absorption`` (alpha, as in ``gmres``): the lossy operator in the float64 residual, the fp32 cycle and the preconditioner
        (``helmnet_amd.gmres.gmres_refine_lossy``, hn_fgmres_refine_cycle_lossy); the same dictionary comes back.  None: the code path and the bits
        of before."""
        from .gmres import gmres, gmres_refine_lossy
        if absorption is not None:
            self._refuse_medium_grad("gmres64", False, sos_maps, absorption, x0)
            self._require_square("gmres64")
            return gmres_refine_lossy(self, sos_maps, absorption, restart=restart, max_outer=max_cycles, tol=tol, x0=x0, precondition=precondition,
                                      precond_iterations=precond_iterations, precond_scale=precond_scale)
        self._require_square("gmres64")
        return gmres(self, sos_maps, restart=restart, max_outer=max_cycles, tol=tol, x0=x0, backend="hip", refine=True, precondition=precondition,
                     precond_iterations=precond_iterations, precond_scale=precond_scale)

    def adjoint_solve(self, cotangent, sos, precondition: Optional[str] = "learned", **kwargs) -> dict:
        """Solve the adjoint system A^H lam = ``cotangent`` [B or 1,2,n,n] (dJ/du as two real planes) on the maps ``sos`` [B,1,n,n]: restarted GMRES on
        the conjugate transpose of ``gmres``'s operator (``helmnet_amd.gmres.gmres_adjoint``, whose keyword arguments pass through).
        ``precondition="learned"`` (the default here: measured faster than the plain cycle at 96^2 and at 256^2): the flexible cycle
        with this solver's network between the similarity weight W; None: plain restarted GMRES.  ``out["wavefield"]`` is lam.  No gradients.
        ``absorption=alpha`` among the keyword arguments: the adjoint of the lossy operator (hn_fgmres_adjoint_cycle_lossy); ``density=rho``: the
        adjoint of the variable-density operator (hn_fgmres_adjoint_cycle_medium), with or without absorption."""
        from .gmres import gmres_adjoint
        self._require_square("adjoint_solve")
        return gmres_adjoint(self, sos, cotangent, precondition=precondition, **kwargs)

    def solve_implicit(self, sos, tol: float = 1e-4, adjoint_tol: Optional[float] = None, restart: int = 20, max_cycles: int = 50,
                       precondition: Optional[str] = "learned", precond_iterations: int = 10, x0=None, absorption=None, density=None) -> dict:
        """The solution of A u = source to ``tol`` with the gradient of the SOLUTION, by the adjoint-state method: the forward solve is ``gmres`` (fused
        cycles on the device, under no_grad on detached inputs, nothing taped), and ``out["wavefield"]`` carries one autograd node whose backward solves
        A^H lam = dJ/du to ``adjoint_tol`` (default ``tol``; ``adjoint_solve`` with the same restart, max_cycles, precondition and precond_iterations),
        forms dJ/dk_sq = -Re(conj(lam) u) and dJ/dsource = lam (hn_adjoint_grad) and chains to ``sos`` (k_sq = (omega / sos)^2) and to ``self.source``
        where they require grad.  One extra linear solve and O(1) memory whatever converged u; the weights get no gradient (u does not depend on them).
        Returns the dictionary of ``gmres`` plus ``"adjoint"``: a dictionary filled by backward with cycles, rmse (final true RMSE per sample),
        converged, iterations and unet_evaluations of the adjoint solve.  Square domains; 16-bit UNet precision modes are allowed (the network
        only preconditions).  ``create_graph=True`` raises RuntimeError.
        ``absorption`` (alpha, as in ``gmres``): the medium is lossy.  The forward solve is ``gmres(..., absorption=...)`` on detached inputs, and the
        one autograd node solves the lossy adjoint system (hn_fgmres_adjoint_cycle_lossy), forms dJ/dk_sq, dJ/dk_sq_im and dJ/dsource
        (hn_adjoint_grad_lossy) and chains through ``absorption.complex_k_sq`` to ``sos``, to ``absorption`` when it is a tensor that requires grad
        (summed over the dimensions it broadcasts along) and to ``self.source``.  A number gets no gradient.  None: the code path and the bits of
        before.
        ``density`` (rho, a tensor broadcastable to ``sos``, as in ``gmres``): the medium has a heterogeneous density, with or without ``absorption``.
        The forward solve is ``gmres(..., density=...)`` on detached inputs; the one autograd node solves A_rho^H lam = dJ/du
        (hn_fgmres_adjoint_cycle_medium), forms dJ/dk_sq, dJ/dk_sq_im, dJ/dq and dJ/dsource in one call (hn_adjoint_grad_medium) and chains to
        ``sos``, to ``absorption``, to ``density`` when it requires grad (``density.log_density_gradient_vjp``, summed to its own shape) and to
        ``self.source``.  None: the code path and the bits of before."""
        from .autograd import SolveImplicit, SolveImplicitLossy, SolveImplicitMedium
        from .gmres import gmres
        self._require_square("solve_implicit")
        n = int(self.hparams.domain_size)
        if not isinstance(sos, torch.Tensor) or sos.dim() != 4 or tuple(sos.shape[1:]) != (1, n, n):
            raise ValueError(f"sos must be [B, 1, {n}, {n}], got {tuple(getattr(sos, 'shape', ()))}")
        if self.source.shape[0] not in (1, sos.shape[0]):
            raise ValueError(f"the solver holds {self.source.shape[0]} source maps for a batch of {sos.shape[0]}")
        if x0 is not None and tuple(x0.shape) != (sos.shape[0], 2, n, n):
            raise ValueError(f"x0 must be [{sos.shape[0]}, 2, {n}, {n}], got {tuple(x0.shape)}")
        if precondition not in (None, "learned"):
            raise ValueError(f"unknown precondition {precondition!r} (choose None or 'learned')")
        alpha = None
        if absorption is not None:
            alpha = absorption if isinstance(absorption, torch.Tensor) else torch.as_tensor(float(absorption))
            try:
                fits = tuple(torch.broadcast_shapes(tuple(alpha.shape), tuple(sos.shape))) == tuple(sos.shape)
            except RuntimeError:
                fits = False
            if not fits:
                raise ValueError(f"absorption of shape {tuple(alpha.shape)} does not broadcast to sos {tuple(sos.shape)}")
        if density is not None:
            if not isinstance(density, torch.Tensor):
                raise TypeError("density must be a tensor broadcastable to the sound-speed maps")
            try:
                fits = density.dim() == 4 and tuple(torch.broadcast_shapes(tuple(density.shape), tuple(sos.shape))) == tuple(sos.shape)
            except RuntimeError:
                fits = False
            if not fits:
                raise ValueError(f"density of shape {tuple(density.shape)} does not broadcast to sos {tuple(sos.shape)}")
        common = dict(restart=int(restart), precondition=precondition, precond_iterations=int(precond_iterations))
        lossy = {} if alpha is None else {"absorption": alpha.detach()}
        if density is not None:
            lossy["density"] = density.detach()
        with torch.no_grad():
            out = gmres(self, sos.detach(), max_outer=int(max_cycles), tol=float(tol), x0=None if x0 is None else x0.detach(), backend="hip", **common,
                        **lossy)
        info: dict = {}
        spec = {"solver": self, "wavefield": out["wavefield"], "info": info,
                "adjoint_kwargs": dict(common, max_outer=int(max_cycles), tol=float(tol if adjoint_tol is None else adjoint_tol))}
        if density is not None:
            dev = out["wavefield"].device
            spec["lossy"] = alpha is not None
            a = torch.zeros((), device=dev) if alpha is None else alpha.to(dev).float()
            out["wavefield"] = SolveImplicitMedium.apply(spec, sos.to(dev).float(), a, density.to(dev).float(), self._src_graph())
        elif alpha is None:
            out["wavefield"] = SolveImplicit.apply(spec, sos.float(), self._src_graph())
        else:
            dev = out["wavefield"].device
            out["wavefield"] = SolveImplicitLossy.apply(spec, sos.to(dev).float(), alpha.to(dev).float(), self._src_graph())
        out["adjoint"] = info
        return out

    def reference_error(self, wavefield, sos_maps, tol: float = 1e-10, restart: int = 20, max_cycles: int = 400, precondition=None,
                        precond_iterations: int = 10, precond_scale=None, absorption=None) -> dict:
        """How far ``wavefield`` [B,2,n,n] is from the solution of the discrete problem: ``gmres64`` started from it is the ground truth.  Returns per
        sample ``linf`` (max |wavefield - reference| over both planes) and ``rms`` of the same difference, ``reference_rmse64`` (the float64
        residual RMSE of the reference: how good the ground truth is; below ``tol`` when ``converged``), ``reference`` (the float64 wavefield),
        ``converged`` and ``cycles``.  ``wavefield`` is not written.  ``absorption``: the lossy problem, as in ``gmres64``."""
        if absorption is not None:
            self._refuse_medium_grad("reference_error", False, wavefield, sos_maps, absorption)
        _require_no_grad("reference_error", wavefield, sos_maps)
        self._require_square("reference_error")
        lossy = {} if absorption is None else {"absorption": absorption}
        out = self.gmres64(sos_maps, restart=restart, max_cycles=max_cycles, tol=tol, x0=wavefield, precondition=precondition,
                           precond_iterations=precond_iterations, precond_scale=precond_scale, **lossy)
        ref = out["wavefield"]
        diff = wavefield.detach().to(ref.device).double() - ref
        return {"linf": diff.abs().amax((1, 2, 3)), "rms": diff.pow(2).mean((1, 2, 3)).sqrt(), "reference_rmse64": out["residual_norm64"],
                "reference": ref, "converged": out["converged"], "cycles": out["cycles"]}

    def solve_many(self, sos_maps, tol: float, max_iterations: int = None, slots: int = 32, check_every: int = 25,
                   source_maps=None, diverge_rmse: float = None, keep_residuals: bool = False, norm_reduce=None) -> dict:
        """Extension: solve a stream of N maps to a tolerance, every map stopping on its own (continuous batching; the workload of the
        reference's evaluate.py, which runs its test set batch by batch for a fixed iteration count).  ``slots`` maps iterate at a time
        in chunks of ``check_every``; after each chunk one launch judges every slot from the chunk's RMSE rows (``hn_stream_verdict``),
        the host synchronises once, and one launch (``hn_stream_swap``) retires finished slots into the outputs, hands them the next
        unsolved maps and, when none is left, moves the last active slots into the holes -- ``hn_step`` always runs a dense prefix.

        ``sos_maps`` [N,1,n,n], any N (a host tensor is uploaded whole, once); ``source_maps`` None: the solver's one source map
        (``self.source`` must be [1,2,n,n]), or [N,2,n,n], one per map.  A map is retired after the chunk in which its residual RMSE is
        NaN / Inf or above ``diverge_rmse`` (status 2), else in which it was below ``tol`` at some iteration (status 0), else when it has
        run ``max_iterations`` (status 1).  CHUNK GRANULARITY: the stop is decided per chunk and no extra history is kept, so the
        wavefield and ``residual_norm`` returned are those at the END of that chunk and ``iterations`` is a multiple of ``check_every``
        capped at ``max_iterations`` (helmnet_amd.stream_schedule has the rule for a ``max_iterations`` that is not a multiple); a
        residual that dips below ``tol`` and rises again inside the chunk is reported as converged with the larger end-of-chunk norm.

        Returns ``wavefields`` [N,2,n,n], ``residual_norm`` [N] (device), ``iterations`` int64 [N], ``status`` int8 [N] (host; 0 converged,
        1 hit max_iterations, 2 diverged / non-finite), ``residuals`` [N,2,n,n] with ``keep_residuals``, ``sample_iterations`` (the sum over
        chunks of active slots x chunk length: the work enqueued) and ``chunks``.  With ``slots`` <= 32 every map's result is bit-identical
        to ``forward(sos[m:m+1], num_iterations=iterations[m])`` (fp32 UNet; INTEGRATION.md section 7 says where that stops holding).
        ``norm_reduce`` (e.g. helmnet_amd.distributed.allreduce_residual_norms) is called ONCE, at the end, on the final norms
        (``worst_residual_norm``): ranks stream their shards independently.  Runs without gradients -- an input that requires grad raises
        (the differentiable path is ``forward``) -- and leaves the hidden states held in ``f`` untouched."""
        import numpy as np
        from .stream_schedule import StreamScheduler
        if max_iterations is None:
            max_iterations = self.hparams.max_iterations
        _require_no_grad("solve_many", sos_maps, source_maps)
        self._require_square("solve_many")
        if not (float(tol) == float(tol)):
            raise ValueError("tol is NaN")
        with torch.no_grad():
            eng = self.engine()
            dev, n = eng.device, int(self.hparams.domain_size)
            if sos_maps.dim() != 4 or tuple(sos_maps.shape[1:]) != (1, n, n):
                raise ValueError(f"sos_maps must be [N, 1, {n}, {n}], got {tuple(sos_maps.shape)}")
            N = int(sos_maps.shape[0])
            sos_in = sos_maps.detach().to(dev, torch.float32).contiguous()
            if source_maps is None:
                src_in, src = None, self._src()
                if src.shape[0] != 1:
                    raise ValueError(f"the solver holds {src.shape[0]} source maps: pass source_maps=[N, 2, {n}, {n}] (one per map)")
            else:
                if tuple(source_maps.shape) != (N, 2, n, n):
                    raise ValueError(f"source_maps must be [{N}, 2, {n}, {n}], got {tuple(source_maps.shape)}")
                src_in = source_maps.detach().to(dev, torch.float32).contiguous()
            sched = StreamScheduler(N, slots, max_iterations, check_every)
            new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
            out_wf = new(N, 2, n, n)
            out_res = new(N, 2, n, n) if keep_residuals else None
            S = min(sched.slots, N)
            if S > 0:
                eng.reserve(S)
                wf, res, st, k_sq = new(S, 2, n, n), new(S, 2, n, n), new(S, 2, eng.state_len), new(S, 1, n, n)
                if src_in is not None:
                    src = new(S, 2, n, n)
                rmse = new(sched.check_every * S)
                omega = float(self.hparams.omega)
                per_slot = src_in is not None
                stream = torch.cuda.current_stream(dev)
                eng.stream_swap(wf, res, st, k_sq, src, sched.initial_ops(), sos_in, src_in, omega)
                while sched.active:
                    a, chunk = sched.active, sched.next_chunk()
                    hist = rmse[: chunk * a].view(chunk, a)
                    eng.step(wf[:a], res[:a], st[:a], k_sq[:a], src[:a] if per_slot else src, chunk, rmse_hist=hist)
                    table = eng.stream_verdict(hist, tol, diverge_rmse)
                    stream.synchronize()
                    eng.check_async_errors()
                    ops = sched.advance(chunk, table.tolist())
                    eng.stream_swap(wf, res, st, k_sq, src, ops, sos_in, src_in, omega, out_wf, out_res)
            norms = torch.tensor(np.asarray(sched.residual_norm, dtype=np.float32), device=dev)
            out = {"wavefields": out_wf, "iterations": torch.tensor(sched.iterations, dtype=torch.int64),
                   "residual_norm": norms, "status": torch.tensor(sched.status, dtype=torch.int8),
                   "sample_iterations": sched.sample_iterations, "chunks": sched.chunks}
            if keep_residuals:
                out["residuals"] = out_res
            if norm_reduce is not None:
                out["worst_residual_norm"] = norm_reduce(norms, "max")
            return out

    def forward_variable_src(self, sos_maps, src_time_pairs, return_wavefields=False, return_states=False,
                             num_iterations=None, stop_if_diverge=False, residuals: str = "all"):
        """hybridnet.py:699-754: swap the source map at given iterations (the residual is recomputed
        with the new source before the step, states and wavefield carry over)."""
        if num_iterations is None:
            num_iterations = self.hparams.max_iterations
        times = list(src_time_pairs["iteration"])
        maps = iter(src_time_pairs["src_maps"])
        sos_maps = sos_maps.float().contiguous()
        k_sq, wf = self.get_initials(sos_maps)
        self.f.clear_states(wf)
        res = self.get_residual(wf, k_sq)
        st = self.f.get_states(flatten=True).contiguous()
        cuts = sorted(set(t for t in times if 0 <= t < num_iterations) | {0, num_iterations})
        merged = {"wavefields": [], "residuals": [], "states": [], "last_iteration": num_iterations - 1}
        norms: List[torch.Tensor] = []
        for a, bnd in zip(cuts[:-1], cuts[1:]):
            if a in times:
                self.set_source_maps(next(maps))
                res = self.get_residual(wf, k_sq)
            part = self._run(wf, res, st, Medium(k_sq), bnd - a, return_wavefields, return_states, residuals)
            if residuals == "all":
                merged["residuals"] += part["residuals"]
            merged["states"] += part["states"]
            if return_wavefields:
                merged["wavefields"] += part["wavefields"]
            norms.append(part["residual_norms"])
        if not return_wavefields:
            merged["wavefields"].append(wf)
        if residuals == "last":      # wf / res / st are updated in place by every segment: only the final ones are kept
            merged["residuals"] = [res]
        elif residuals == "norms":
            merged["last_residual"] = res
        merged["residual_norms"] = torch.cat(norms, 0) if norms else None
        return merged
