"""Thin tensor-level wrapper over one ``hn_ctx`` of libhelmnet_hip.so.

PyTorch is used for device memory and streams only: every method checks its tensors
(device, dtype, contiguity, shape), passes raw device pointers plus the current HIP stream
across the C ABI, and returns.  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib

# state_dict order of the `f.*` tensors = order of the blob hn_load_weights expects
# (reference helmnet/architectures.py:317-388)


def weight_names(depth: int = 4) -> list:
    def dc(prefix):
        p = prefix + ".double_conv."
        return [p + "0.weight", p + "0.bias", p + "1.weight", p + "2.weight", p + "2.bias"]

    names = dc("inc")
    for d in range(depth):
        names += dc(f"enc.{d}.conv_signal") + [f"enc.{d}.down.weight", f"enc.{d}.down.bias"] + dc(f"enc.{d}.conv_state")
    for d in range(depth + 1):
        names += dc(f"decode.{d}")
    for d in range(depth):
        names += [f"up.{d}.weight", f"up.{d}.bias"]
    return names + ["outc.conv.weight", "outc.conv.bias"]


def pack_weights(state: dict, depth: int = 4, activation: str = "prelu", state_depth: Optional[int] = None) -> np.ndarray:
    """Flatten a HybridNet state_dict (tensors or arrays) into the fp32 blob of hn_load_weights.
    Parameter-free activations (relu / leakyrelu) get their constant slope written where the
    PReLU weight would be, so the blob layout never changes.

    ``state_depth < depth`` (architectures.py:353, ``use_state = d < state_depth``): the kernels always run the stateful
    layout, so an encoder level WITHOUT state is packed as its exact stateful equivalent -- conv_signal's first
    convolution [8, 8, 3, 3] gets two all-zero input channels where the state would be concatenated (their products are
    exact zeros), and the missing conv_state becomes an all-zero DoubleConv; the host leaves that level's state slice
    untouched (HybridNet.adopt_states)."""
    const_slope = {"relu": 0.0, "leakyrelu": 0.01, "celu": 0.0, "tanh": 0.0, "gelu": 0.0, "tanhshrink": 0.0, "softplus": 0.0}
    state_depth = depth if state_depth is None else state_depth
    stateless = {f"enc.{d}." for d in range(state_depth, depth)}
    zero_state_dc = {"0.weight": (2, 10, 3, 3), "0.bias": (2,), "2.weight": (2, 2, 3, 3), "2.bias": (2,)}
    parts = []
    for name in weight_names(depth):
        level = name[: name.index(".", 4) + 1] if name.startswith("enc.") else None
        if level in stateless and ".conv_state." in name:
            tail = name.split(".double_conv.")[1]
            parts.append(np.full(1, 0.25, np.float32) if tail == "1.weight" else np.zeros(int(np.prod(zero_state_dc[tail])), np.float32))
            continue
        if name.endswith(".double_conv.1.weight") and name not in state:
            if activation.lower() not in const_slope:
                raise KeyError(f"missing {name} for activation {activation!r}")
            parts.append(np.array([const_slope[activation.lower()]], np.float32))
            continue
        v = state[name]
        if isinstance(v, torch.Tensor):
            v = v.detach().to("cpu", torch.float32).numpy()
        v = np.ascontiguousarray(v, dtype=np.float32)
        if level in stateless and name.endswith(".conv_signal.double_conv.0.weight"):
            assert v.shape[1] == 8, v.shape
            v = np.concatenate([v, np.zeros((v.shape[0], 2, 3, 3), np.float32)], 1)
        parts.append(v.reshape(-1))
    return np.concatenate(parts)


def weight_shapes(depth: int = 4, features: int = 8, state_channels: int = 2, inchannels: int = 6) -> dict:
    """name -> shape of every tensor of the blob, in blob order (architectures.py:63-84, 209-211, 340-388)."""
    f, s = features, state_channels

    def dc(prefix, cin, cm, co):
        p = prefix + ".double_conv."
        return {p + "0.weight": (cm, cin, 3, 3), p + "0.bias": (cm,), p + "1.weight": (1,), p + "2.weight": (co, cm, 3, 3), p + "2.bias": (co,)}

    shapes = dc("inc", inchannels, f, f)
    for d in range(depth):
        shapes.update(dc(f"enc.{d}.conv_signal", f + s, f, f))
        shapes.update({f"enc.{d}.down.weight": (f, f, 8, 8), f"enc.{d}.down.bias": (f,)})
        shapes.update(dc(f"enc.{d}.conv_state", f + s, s, s))
    for d in range(depth + 1):
        shapes.update(dc(f"decode.{d}", 2 * f if d < depth else f, f, f))
    for d in range(depth):
        shapes.update({f"up.{d}.weight": (f, f, 8, 8), f"up.{d}.bias": (f,)})
    shapes.update({"outc.conv.weight": (2, f, 1, 1), "outc.conv.bias": (2,)})
    assert list(shapes) == weight_names(depth)
    return shapes


def unpack_weights(blob, depth: int = 4) -> dict:
    """Inverse of pack_weights for state_depth == depth: flat fp32 blob (array or tensor) -> {name: array in PyTorch layout}."""
    if isinstance(blob, torch.Tensor):
        blob = blob.detach().to("cpu", torch.float32).numpy()
    out, pos = {}, 0
    for name, shape in weight_shapes(depth).items():
        n = int(np.prod(shape))
        out[name] = np.array(blob[pos:pos + n], np.float32).reshape(shape)
        pos += n
    assert pos == blob.size, (pos, blob.size)
    return out


_MODULE_ENGINES: dict = {}


def module_engine(device) -> "Engine":
    """One shared context per device for the standalone sub-module forwards (DoubleConv / OutConv / EncoderBlock called directly)."""
    dev = torch.device(device)
    dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device()) if dev.type == "cuda" else dev
    if dev not in _MODULE_ENGINES:
        _MODULE_ENGINES[dev] = Engine(dev)
    return _MODULE_ENGINES[dev]


def release_module_engines():
    """Destroy the shared per-device contexts of the standalone sub-module forwards (they otherwise live until interpreter exit)."""
    for eng in _MODULE_ENGINES.values():
        eng.close()
    _MODULE_ENGINES.clear()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _require_no_grad(what: str, *tensors):
    """The one refusal of every entry that computes without autograd (the float64 loop and residual, GMRES, solve_many)."""
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.requires_grad:
            raise RuntimeError(f"{what} runs without gradients: pass detached tensors (the differentiable path is forward())")


def _tensor(t, name: str) -> torch.Tensor:
    """The plane a ``*_lossy`` / ``*_medium`` method cannot do without (None would name another kind of medium)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    return t


class Medium(NamedTuple):
    """What multiplies the wavefield beside the Laplacian: ``k_sq`` [B,1,h,w], for an absorbing medium its imaginary part ``k_sq_im`` [B,1,h,w], for a
    heterogeneous density ``rho_grad`` [B,2,h,w] (and then ``k_sq_im`` or None).  A public method builds it, everything below passes it on."""
    k_sq: torch.Tensor
    k_sq_im: Optional[torch.Tensor] = None
    rho_grad: Optional[torch.Tensor] = None

    @property
    def kind(self) -> str:
        """The suffix of the library's entry points for this medium: ``hn_step`` + kind, ``hn_residual`` + kind, ..."""
        return "_medium" if self.rho_grad is not None else "_lossy" if self.k_sq_im is not None else ""

    def planes(self) -> tuple:
        """The medium as the methods and entry points of its kind take it, in k_sq's place: their signatures differ only there."""
        return {"": self[:1], "_lossy": self[:2], "_medium": self[:3]}[self.kind]


class Engine:
    """One library context bound to one HIP device."""

    def __init__(self, device: torch.device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.HelmnetHipError(
                f"helmnet_amd computes on MI355X (device type 'cuda' under ROCm) only, got {device}; "
                "there is no CPU path in the product (the CPU oracle lives in oracle/ for tests)."
            )
        self.lib = _lib.load()
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        ctx = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            torch.cuda.current_stream()  # make sure torch initialised HIP on this device first
            _lib.check(self.lib.hn_create(ctypes.byref(ctx), self.device.index), None, "hn_create")
        self.ctx = ctx
        self.n = 0                # side of a square domain; 0 without a domain and on a rectangular one
        self.hw = (0, 0)          # (rows, columns) of the domain
        self.depth = 0
        self.weights_key = None
        self.domain_key = None

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.hn_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup -------------------------------------------------------------------------
    def load_weights(self, blob: np.ndarray, features: int, depth: int, state_channels: int, activation: str):
        act = _lib.HN_ACT.get(activation.lower())
        if act is None:
            raise NotImplementedError(f"Unknown activation function {activation} (HIP kernels: {sorted(_lib.HN_ACT)})")
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        rc = self.lib.hn_load_weights(self.ctx, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), blob.size,
                                      features, depth, state_channels, act)
        _lib.check(rc, self.ctx, "hn_load_weights")
        self.depth = depth

    def set_domain(self, n: int, pml: int, sigma_max: float, k: float):
        _lib.check(self.lib.hn_set_domain(self.ctx, int(n), int(pml), float(sigma_max), float(k)), self.ctx, "hn_set_domain")
        self.n = int(n)
        self.hw = (int(n), int(n))
        self.domain_key = (int(n), int(pml), float(sigma_max), float(k))

    def set_domain_rect(self, h: int, w: int, pml: int, sigma_max: float, k: float):
        """An h x w domain (hn_set_domain_rect): h rows by w columns, tensors [B, C, h, w].  h == w is ``set_domain(h, ...)`` itself.  On h != w the
        operators, ``unet`` and ``step`` work in the 'fp32' and 'valu' precision modes, and ``residual64_lossy`` in float64; every other method that reads the domain raises
        NotImplementedError naming the rectangular domain.  ``domain_key`` carries both sizes: ((h, w), pml, sigma_max, k)."""
        if int(h) == int(w):
            return self.set_domain(h, pml, sigma_max, k)
        _lib.check(self.lib.hn_set_domain_rect(self.ctx, int(h), int(w), int(pml), float(sigma_max), float(k)), self.ctx, "hn_set_domain_rect")
        self.n = 0
        self.hw = (int(h), int(w))
        self.domain_key = ((int(h), int(w)), int(pml), float(sigma_max), float(k))

    def set_unet_precision(self, mode: str):
        """Arithmetic of the UNet convolutions for this context: 'fp32' (default), 'bf16x3', 'fp16', 'bf16x2', 'valu'."""
        if mode not in _lib.HN_PRECISION:
            raise ValueError(f"unknown UNet precision {mode!r} (choose from {sorted(_lib.HN_PRECISION)})")
        _lib.check(self.lib.hn_set_unet_precision(self.ctx, _lib.HN_PRECISION[mode]), self.ctx, "hn_set_unet_precision")

    @property
    def unet_precision(self) -> str:
        code = self.lib.hn_get_unet_precision(self.ctx)
        names = {v: k for k, v in _lib.HN_PRECISION.items()}
        if code not in names:
            raise _lib.HelmnetHipError(f"hn_get_unet_precision returned {code} (context closed?)")
        return names[code]

    def set_option(self, name: str, value: int):
        """Library tuning knobs (enum hn_option of include/helmnet_hip.h): 'lanes' 1..8, 'side_stream' 0..3, 'deep' 0/1, 'spectral_pfa' 0/1,
        'spectral_radix16' 0..2, 'dc_valu' 0..4, 'spectral_cols' 0..3, 'train_fused', 'train_overlap', 'mc_stage' 0/1 (the matrix-core 8x8 / strip kernels with
        the input staging behind the MFMAs; bit-identical), 'module_mc' 0/1 (default 0; 1: double_conv with 8 output channels and conv8x8 run on the
        network's own dispatch -- the matrix-core / vector-pipe kernels the precision mode, 'dc_valu' and 'mc_stage' select -- instead of the direct
        kernels; module_route names the instance); laboratory knobs (HN_EXP_*): 'graph' 0, 1 or an even
        number <= 64 of iterations per graph, 'train_lanes' 1/2 (hn_train_grad: the halves of the batch as two chains of launches on two streams).
        'spectral_pfa' and 'spectral_mixed' 0/1 (FFT for every other size P * 2^k, P odd; default 0) are read when the spectral tables are built:
        changing one re-builds them; counter('spectral_route') tells which kernels the domain runs on (1 power of two, 2 prime-factor, 3 dense,
        4 mixed, 5 rectangular).
        'spectral_cols' 0..2 is bit-exact: for a fixed 'spectral_radix16' these three column kernels give the same bits (with 'spectral_radix16' 0 it
        is not read); 3 is another factorisation (fp32 rounding).  'spectral_plain' (laboratory knob) 1: the 256- / 512-point kernel bodies instantiated on
        plain C++ complex helpers (k_spec*_plain), bit-identical to 0.  'spectral_radix16' and 'spectral_pfa' select other kernels for the same fp32 arithmetic: results agree to fp32 rounding (every
        combination is within 1e-6 of the operator's scale of the float64 oracle, the dense operator within 7e-6), not bit for bit.  Neither makes a
        sample's result depend on what shares its batch (tests/test_spectral_gpu.py).
        'f64_fft' 0/1 (default 0) picks the route of the float64 operator (laplacian64, residual64, step64, the refine cycles): 0 the dense kernel, 1 two
        FFT line passes in double (laplacian.f64_route).  It is read by every float64 call, needs no table re-build and can be flipped between calls;
        the routes agree to float64 rounding (2e-11 of the scale), not bit for bit; counter('f64_route') tells which one the last float64 call on the
        domain took (0 none yet, 1 dense, 2 FFT)."""
        if name not in _lib.HN_OPTION:
            raise ValueError(f"unknown option {name!r} (choose from {sorted(_lib.HN_OPTION)})")
        _lib.check(self.lib.hn_set_option(self.ctx, _lib.HN_OPTION[name], int(value)), self.ctx, "hn_set_option")
        if name in ("spectral_pfa", "spectral_mixed") and self.domain_key is not None and self.n:   # (a rectangular domain reads neither)
            self.set_domain(*self.domain_key)

    def counter(self, name: str) -> int:
        return int(self.lib.hn_get_counter(self.ctx, _lib.HN_COUNTER[name]))

    def check_async_errors(self):
        """Raise if a bounded device-side wait of any earlier call on this context gave up (hn_check_async_errors); reliable once the stream the work
        ran on has been synchronised."""
        _lib.check(self.lib.hn_check_async_errors(self.ctx), self.ctx, "hn_check_async_errors")

    @property
    def state_len(self) -> int:
        return int(self.lib.hn_state_len(self.ctx))

    def reserve(self, batch: int):
        _lib.check(self.lib.hn_reserve(self.ctx, int(batch)), self.ctx, "hn_reserve")

    # ---- helpers -----------------------------------------------------------------------
    def _chk(self, t: torch.Tensor, shape: Sequence[int], name: str, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if t.device != self.device:
            raise ValueError(f"{name} is on {t.device}, engine is on {self.device}")
        if t.dtype != dtype:
            raise TypeError(f"{name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return t

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- operators ---------------------------------------------------------------------
    def sigmas(self) -> torch.Tensor:
        out = torch.empty(2, *self.hw, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.hn_get_sigmas(self.ctx, _ptr(out), self._stream()), self.ctx, "hn_get_sigmas")
        return out

    def laplacian(self, wf: torch.Tensor) -> torch.Tensor:
        b = wf.shape[0]
        self._chk(wf, (b, 2, *self.hw), "wavefield")
        out = torch.empty_like(wf)
        _lib.check(self.lib.hn_laplacian(self.ctx, _ptr(wf), _ptr(out), b, self._stream()), self.ctx, "hn_laplacian")
        return out

    def _call(self, stem: str, m: Medium, before: list, after: list):
        """The entry point ``stem`` + the medium's kind, the medium's pointers between ``before`` and ``after``."""
        name = stem + m.kind
        _lib.check(getattr(self.lib, name)(self.ctx, *before, *map(_ptr, m.planes()), *after, self._stream()), self.ctx, name)

    def _chk_medium(self, m: Medium, b: int, dtype: torch.dtype = torch.float32) -> None:
        self._chk(m.k_sq, (b, 1, *self.hw), "k_sq", dtype)
        if m.k_sq_im is not None:
            self._chk(m.k_sq_im, (b, 1, *self.hw), "k_sq_im", dtype)
        if m.rho_grad is not None:
            self._chk(m.rho_grad, (b, 2, *self.hw), "rho_grad", dtype)

    def _residual(self, m: Medium, wf: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
        b = wf.shape[0]
        self._chk(wf, (b, 2, *self.hw), "wavefield")
        self._chk_medium(m, b)
        self._chk(src, (src.shape[0], 2, *self.hw), "source")
        out = torch.empty_like(wf)
        self._call("hn_residual", m, [_ptr(wf)], [_ptr(src), src.shape[0], _ptr(out), b])
        return out

    def residual(self, wf: torch.Tensor, k_sq: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
        return self._residual(Medium(k_sq), wf, src)

    def _residual_vjp(self, m: Medium, g: torch.Tensor) -> torch.Tensor:
        b = g.shape[0]
        self._chk(g, (b, 2, *self.hw), "cotangent")
        self._chk_medium(m, b)
        out = torch.empty_like(g)
        self._call("hn_residual_vjp", m, [_ptr(g)], [_ptr(out), b])
        return out

    def residual_vjp(self, g: torch.Tensor, k_sq: torch.Tensor) -> torch.Tensor:
        """J^T g of ``residual`` with respect to the wavefield: L^H(g) + k_sq * g."""
        return self._residual_vjp(Medium(k_sq), g)

    def rmse(self, res: torch.Tensor) -> torch.Tensor:
        b = res.shape[0]
        self._chk(res, (b, 2, *self.hw), "residual")
        out = torch.empty(b, device=self.device, dtype=torch.float32)
        _lib.check(self.lib.hn_rmse(self.ctx, _ptr(res), _ptr(out), b, self._stream()), self.ctx, "hn_rmse")
        return out

    def _gmres_buffers(self, what: str, x, x_dtype, m: Medium, rhs, restart: int, basis, hess):
        """What the cycle methods share: the grad refusal, the shape checks, ``basis`` / ``hess`` (allocated when not given) and the fresh ``rmse``
        [restart + 1, B] and ``k_used`` [B] int32 tables."""
        b, p2 = x.shape[0], 2 * self.hw[0] * self.hw[1]
        for t, name in ((x, "x"), (m.k_sq, "k_sq"), (rhs, "rhs"), (m.k_sq_im, "k_sq_im"), (m.rho_grad, "rho_grad")):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise RuntimeError(f"{what}: {name} requires grad; the GMRES cycle is not differentiable")
        self._chk(x, (b, 2, *self.hw), "x", x_dtype)
        self._chk_medium(m, b)
        self._chk(rhs, (rhs.shape[0], 2, *self.hw), "rhs")
        new = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)  # noqa: E731
        basis = self._chk(new(b, restart + 1, p2) if basis is None else basis, (b, restart + 1, p2), "basis")
        hess = self._chk(new(b, restart + 1, restart, 2) if hess is None else hess, (b, restart + 1, restart, 2), "hess")
        return b, basis, hess, new(restart + 1, b), torch.empty(b, device=self.device, dtype=torch.int32)

    def _zbasis(self, b: int, restart: int, zbasis):
        """The flexible cycles' ``zbasis`` [B, restart, 2 n^2], allocated when not given."""
        shape = (b, restart, 2 * self.hw[0] * self.hw[1])
        return self._chk(torch.empty(shape, device=self.device, dtype=torch.float32) if zbasis is None else zbasis, shape, "zbasis")

    def gmres_cycle(self, x: torch.Tensor, k_sq: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float,
                    basis: Optional[torch.Tensor] = None, hess: Optional[torch.Tensor] = None):
        """One restart cycle of GMRES(restart) on A u = L(u) + k_sq * u (hn_gmres_cycle), ``x`` updated in place, nothing synchronised.  Returns
        (rmse [restart + 1, B], k_used [B] int32): row 0 the true residual RMSE of ``x`` at the start, row j the Givens estimate after j inner
        iterations, ``k_used`` the inner iterations that entered each sample's update.  ``basis`` [B, restart + 1, 2 n^2] and ``hess``
        [B, restart + 1, restart, 2] receive the Arnoldi vectors and the Hessenberg matrix; they are allocated when not given."""
        restart = int(restart)
        b, basis, hess, rmse, k_used = self._gmres_buffers("gmres_cycle", x, torch.float32, Medium(k_sq), rhs, restart, basis, hess)
        rc = self.lib.hn_gmres_cycle(self.ctx, _ptr(x), _ptr(k_sq), _ptr(rhs), rhs.shape[0], b, restart, float(tol), _ptr(basis), _ptr(hess),
                                     _ptr(rmse), _ptr(k_used), self._stream())
        _lib.check(rc, self.ctx, "hn_gmres_cycle")
        return rmse, k_used

    def gmres_refine_cycle(self, x: torch.Tensor, k_sq: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float, inner_floor: float = 1e-6,
                           basis: Optional[torch.Tensor] = None, hess: Optional[torch.Tensor] = None):
        """One refinement step of restarted GMRES (hn_gmres_refine_cycle): the true residual of the float64 iterate ``x`` [B,2,n,n] in float64, one fp32
        restart cycle on the scaled correction equation, ``x`` updated in place in float64; nothing synchronised.  ``k_sq`` and ``rhs`` are the fp32
        problem.  Returns (rmse64 [B] float64: the true residual RMSE of ``x`` at the START of the call, rmse [restart + 1, B] and k_used [B] int32:
        the inner cycle's tables, as ``gmres_cycle`` returns them).  A sample with rmse64 < tol is not written and has k_used 0."""
        restart = int(restart)
        b, basis, hess, rmse, k_used = self._gmres_buffers("gmres_refine_cycle", x, torch.float64, Medium(k_sq), rhs, restart, basis, hess)
        rmse64 = torch.empty(b, device=self.device, dtype=torch.float64)
        rc = self.lib.hn_gmres_refine_cycle(self.ctx, _ptr(x), _ptr(k_sq), _ptr(rhs), rhs.shape[0], b, restart, float(tol), float(inner_floor),
                                            _ptr(basis), _ptr(hess), _ptr(rmse), _ptr(k_used), _ptr(rmse64), self._stream())
        _lib.check(rc, self.ctx, "hn_gmres_refine_cycle")
        return rmse64, rmse, k_used

    def fgmres_cycle(self, x: torch.Tensor, k_sq: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float, precond_iters: int, precond_scale: float,
                     basis: Optional[torch.Tensor] = None, hess: Optional[torch.Tensor] = None, zbasis: Optional[torch.Tensor] = None):
        """One FLEXIBLE restart cycle (hn_fgmres_cycle): ``gmres_cycle`` right-preconditioned by the learned iteration -- per inner step
        ``precond_iters`` iterations of ``step`` on A z = precond_scale * v_k from rest, z_k = wf / precond_scale, w = A z_k, and the update over the
        z_j.  Returns (rmse, k_used) as ``gmres_cycle``; ``zbasis`` [B, restart, 2 n^2] (allocated when not given) receives the z_j.
        ``precond_iters`` 0: z = v, ``gmres_cycle`` bit for bit.  Not capturable."""
        return self._fgmres_cycle("hn_fgmres_cycle", Medium(k_sq), x, rhs, restart, tol, precond_iters, precond_scale, basis, hess, zbasis)

    def _fgmres_cycle(self, stem: str, m: Medium, x, rhs, restart, tol, precond_iters, precond_scale, basis, hess, zbasis, rho: tuple = ()):
        """The flexible cycle on A (``stem`` hn_fgmres_cycle) or on A^H (hn_fgmres_adjoint_cycle) for the medium's kind.  ``rho``: empty, or the one
        plane (or None) that hn_fgmres_adjoint_cycle_medium takes behind the medium."""
        restart = int(restart)
        b, basis, hess, rmse, k_used = self._gmres_buffers(stem[3:] + m.kind, x, torch.float32, m, rhs, restart, basis, hess)
        zbasis = self._zbasis(b, restart, zbasis)
        for t in rho:
            if t is not None:
                if t.requires_grad:
                    raise RuntimeError(f"{stem[3:] + m.kind}: rho requires grad; the GMRES cycle is not differentiable")
                self._chk(t, (b, 1, *self.hw), "rho")
        self._call(stem, m, [_ptr(x)], [*map(_ptr, rho), _ptr(rhs), rhs.shape[0], b, restart, float(tol), int(precond_iters), float(precond_scale), _ptr(basis),
                                       _ptr(zbasis), _ptr(hess), _ptr(rmse), _ptr(k_used)])
        return rmse, k_used

    def fgmres_refine_cycle(self, x: torch.Tensor, k_sq: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float, precond_iters: int,
                            precond_scale: float, inner_floor: float = 1e-6, basis: Optional[torch.Tensor] = None,
                            hess: Optional[torch.Tensor] = None, zbasis: Optional[torch.Tensor] = None):
        """One refinement step with the flexible cycle inside (hn_fgmres_refine_cycle): ``gmres_refine_cycle`` with the learned preconditioner of
        ``fgmres_cycle``.  Returns (rmse64, rmse, k_used) as ``gmres_refine_cycle``.  Not capturable."""
        return self._fgmres_refine_cycle(Medium(k_sq), x, rhs, restart, tol, precond_iters, precond_scale, inner_floor, basis, hess, zbasis)

    def _fgmres_refine_cycle(self, m: Medium, x, rhs, restart, tol, precond_iters, precond_scale, inner_floor, basis, hess, zbasis):
        restart = int(restart)
        b, basis, hess, rmse, k_used = self._gmres_buffers("fgmres_refine_cycle" + m.kind, x, torch.float64, m, rhs, restart, basis, hess)
        zbasis = self._zbasis(b, restart, zbasis)
        rmse64 = torch.empty(b, device=self.device, dtype=torch.float64)
        self._call("hn_fgmres_refine_cycle", m, [_ptr(x)], [_ptr(rhs), rhs.shape[0], b, restart, float(tol), float(inner_floor), int(precond_iters),
                                                            float(precond_scale), _ptr(basis), _ptr(zbasis), _ptr(hess), _ptr(rmse), _ptr(k_used),
                                                            _ptr(rmse64)])
        return rmse64, rmse, k_used

    def fgmres_adjoint_cycle(self, x: torch.Tensor, k_sq: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float, precond_iters: int,
                             precond_scale: float, basis: Optional[torch.Tensor] = None, zbasis: Optional[torch.Tensor] = None,
                             hess: Optional[torch.Tensor] = None):
        """One flexible restart cycle on the ADJOINT system A^H x = rhs (hn_fgmres_adjoint_cycle), A^H the operator of ``residual_vjp``: arguments and
        returns as ``fgmres_cycle``.  ``precond_iters`` 0 is plain restarted GMRES on A^H; >= 1 preconditions with the learned iteration between the
        similarity weight of ``laplacian.adjoint_weight``: z_k = conj(W * M(conj(v_k) / W)).  Not capturable."""
        return self._fgmres_cycle("hn_fgmres_adjoint_cycle", Medium(k_sq), x, rhs, restart, tol, precond_iters, precond_scale, basis, hess, zbasis)

    def adjoint_grad(self, lam: torch.Tensor, u: torch.Tensor, src_batch: Optional[int]):
        """The pointwise half of the adjoint-state gradient (hn_adjoint_grad): returns (g_k_sq [B,1,n,n] = -(lam_re u_re + lam_im u_im), g_src) with
        g_src = lam per sample [B,2,n,n] (``src_batch`` == B), its sum over the batch [1,2,n,n] (``src_batch`` == 1) or None (``src_batch`` None)."""
        b = lam.shape[0]
        self._chk(lam, (b, 2, *self.hw), "lam")
        self._chk(u, (b, 2, *self.hw), "u")
        g_k_sq = torch.empty(b, 1, *self.hw, device=self.device, dtype=torch.float32)
        g_src = None if src_batch is None else torch.empty(int(src_batch), 2, *self.hw, device=self.device, dtype=torch.float32)
        rc = self.lib.hn_adjoint_grad(self.ctx, _ptr(lam), _ptr(u), 1 if src_batch is None else int(src_batch), b, _ptr(g_k_sq), _ptr(g_src), self._stream())
        _lib.check(rc, self.ctx, "hn_adjoint_grad")
        return g_k_sq, g_src

    # ---- the same operators in float64: the check the fp32 residual is measured against (hn_f64.hip) ----
    def laplacian64(self, wf: torch.Tensor) -> torch.Tensor:
        b = wf.shape[0]
        self._chk(wf, (b, 2, *self.hw), "wavefield", torch.float64)
        out = torch.empty_like(wf)
        _lib.check(self.lib.hn_laplacian_f64(self.ctx, _ptr(wf), _ptr(out), b, self._stream()), self.ctx, "hn_laplacian_f64")
        return out

    def residual64(self, wf: torch.Tensor, k_sq: torch.Tensor, src: torch.Tensor, want_res: bool = True, want_rmse: bool = True):
        """(res [B,2,n,n] or None, rmse [B] or None), both float64; the RMSE is summed in a fixed order (bit-reproducible)."""
        return self._residual64(Medium(k_sq), wf, src, want_res, want_rmse)

    def _residual64(self, m: Medium, wf, src, want_res: bool, want_rmse: bool):
        b = wf.shape[0]
        self._chk(wf, (b, 2, *self.hw), "wavefield", torch.float64)
        self._chk_medium(m, b, torch.float64)
        self._chk(src, (src.shape[0], 2, *self.hw), "source", torch.float64)
        res = torch.empty_like(wf) if want_res else None
        rmse = torch.empty(b, device=self.device, dtype=torch.float64) if want_rmse else None
        self._call("hn_residual_f64", m, [_ptr(wf)], [_ptr(src), src.shape[0], _ptr(res), _ptr(rmse), b])
        return res, rmse

    # ---- the UNet and the solver loop in float64: the trajectory the fp32 / fp16 / bf16 modes are measured against (hn_unet_f64.hip) ----
    def unet64(self, in6: torch.Tensor, states_in: torch.Tensor):
        """(d [B,2,n,n], states_out [B,2,L]) = HybridNet(in6, states_in) in float64, the weights of the last load_weights up-cast."""
        b = in6.shape[0]
        self._chk(in6, (b, 6, *self.hw), "network input", torch.float64)
        self._chk(states_in, (b, 2, self.state_len), "hidden state", torch.float64)
        d = torch.empty(b, 2, *self.hw, device=self.device, dtype=torch.float64)
        states_out = torch.empty_like(states_in)
        rc = self.lib.hn_unet_f64(self.ctx, _ptr(in6), _ptr(states_in), _ptr(states_out), _ptr(d), b, self._stream())
        _lib.check(rc, self.ctx, "hn_unet_f64")
        return d, states_out

    def step64(self, wf, res, states, k_sq, src, n_iter: int, res_hist=None, wf_hist=None, st_hist=None, rmse_hist=None):
        """n_iter solver iterations in float64; wf, res, states updated in place (``step`` with every tensor float64)."""
        self._step("hn_step_f64", torch.float64, Medium(k_sq), wf, res, states, src, n_iter, res_hist, wf_hist, st_hist, rmse_hist)

    def unet(self, in6: torch.Tensor, states_in: torch.Tensor):
        b = in6.shape[0]
        self._chk(in6, (b, 6, *self.hw), "network input")
        self._chk(states_in, (b, 2, self.state_len), "hidden state")
        d = torch.empty(b, 2, *self.hw, device=self.device, dtype=torch.float32)
        states_out = torch.empty_like(states_in)
        rc = self.lib.hn_unet(self.ctx, _ptr(in6), _ptr(states_in), _ptr(states_out), _ptr(d), b, self._stream())
        _lib.check(rc, self.ctx, "hn_unet")
        return d, states_out

    # ---- standalone sub-modules (hn_double_conv / hn_conv8x8 / hn_out_conv; utility paths, weights re-packed per call) ----
    @staticmethod
    def _host_blob(parts) -> np.ndarray:
        return np.ascontiguousarray(np.concatenate([np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p, np.float32).reshape(-1)
                                                    for p in parts]))

    def _plain(self, x: torch.Tensor, channels: int, name: str) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != channels:
            raise ValueError(f"{name}: expected a [B, {channels}, H, W] tensor, got {tuple(getattr(x, 'shape', ()))}")
        if x.device != self.device:
            raise ValueError(f"{name}: tensor on {x.device}, engine on {self.device}")
        return x.float().contiguous()

    def double_conv(self, x, w1, b1, slope, w2, b2, activation: str = "prelu") -> torch.Tensor:
        """DoubleConv.forward (architectures.py:83-84) for the channel shapes of the UNet."""
        cout, cin = int(w1.shape[0]), int(w1.shape[1])
        x = self._plain(x, cin, "double_conv")
        blob = self._host_blob([w1, b1, np.float32([slope]) if np.isscalar(slope) else slope, w2, b2])
        out = torch.empty(x.shape[0], cout, x.shape[2], x.shape[3], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            rc = self.lib.hn_double_conv(self.ctx, _ptr(x), cin, cout, blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                         _lib.HN_ACT[activation.lower()], _ptr(out), x.shape[0], x.shape[2], x.shape[3], self._stream())
        _lib.check(rc, self.ctx, "hn_double_conv")
        return out

    def conv8x8(self, x, weight, bias, transposed: bool) -> torch.Tensor:
        """nn.Conv2d(8, 8, 8, stride=2, padding=3) / nn.ConvTranspose2d(8, 8, 8, stride=2, padding=3) of the UNet."""
        x = self._plain(x, 8, "conv8x8")
        b, _, h, w = x.shape
        out = torch.empty(b, 8, 2 * h if transposed else h // 2, 2 * w if transposed else w // 2, device=self.device, dtype=torch.float32)
        blob = self._host_blob([weight, bias])
        with torch.cuda.device(self.device):
            rc = self.lib.hn_conv8x8(self.ctx, _ptr(x), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(bool(transposed)), _ptr(out),
                                     b, h, w, self._stream())
        _lib.check(rc, self.ctx, "hn_conv8x8")
        return out

    def module_route(self, op: str, cin: int, h: int, w: int) -> str:
        """The kernel instance (enum hn_route, by its name in _lib.HN_ROUTE) a double_conv ('double_conv'; 'double_conv_smooth' for celu .. softplus) or
        conv8x8 ('down', 'up') call on an h x w input would launch now: hn_module_route, a pure function of the precision mode, the options and the shape."""
        code = int(self.lib.hn_module_route(self.ctx, _lib.HN_ROUTE_OP[op], int(cin), int(h), int(w)))
        _lib.check(min(code, 0), self.ctx, "hn_module_route")
        return {v: k for k, v in _lib.HN_ROUTE.items()}[code]

    def out_conv(self, x, weight, bias) -> torch.Tensor:
        """OutConv.forward (architectures.py:57-60): Conv2d(8, 2, 1)."""
        x = self._plain(x, 8, "out_conv")
        out = torch.empty(x.shape[0], 2, x.shape[2], x.shape[3], device=self.device, dtype=torch.float32)
        blob = self._host_blob([weight, bias])
        with torch.cuda.device(self.device):
            rc = self.lib.hn_out_conv(self.ctx, _ptr(x), blob.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _ptr(out), x.shape[0], x.shape[2],
                                      x.shape[3], self._stream())
        _lib.check(rc, self.ctx, "hn_out_conv")
        return out

    def _step(self, stem: str, dtype, m: Medium, wf, res, states, src, n_iter, res_hist, wf_hist, st_hist, rmse_hist):
        """``step`` on any medium and ``step64``: the checks and the one library call, for tensors of ``dtype``."""
        b = wf.shape[0]
        self._chk(wf, (b, 2, *self.hw), "wavefield", dtype)
        self._chk(res, (b, 2, *self.hw), "residual", dtype)
        self._chk(states, (b, 2, self.state_len), "hidden state", dtype)
        self._chk_medium(m, b, dtype)
        self._chk(src, (src.shape[0], 2, *self.hw), "source", dtype)
        if res_hist is not None:
            self._chk(res_hist, (n_iter, b, 2, *self.hw), "res_hist", dtype)
        if wf_hist is not None:
            self._chk(wf_hist, (n_iter, b, 2, *self.hw), "wf_hist", dtype)
        if st_hist is not None:
            self._chk(st_hist, (n_iter, b, 2, self.state_len), "st_hist", dtype)
        if rmse_hist is not None:
            self._chk(rmse_hist, (n_iter, b), "rmse_hist", dtype)
        self._call(stem, m, [_ptr(wf), _ptr(res), _ptr(states)], [_ptr(src), src.shape[0], b, int(n_iter), _ptr(res_hist), _ptr(wf_hist), _ptr(st_hist),
                                                                 _ptr(rmse_hist)])

    def step(self, wf, res, states, k_sq, src, n_iter: int, res_hist=None, wf_hist=None, st_hist=None, rmse_hist=None):
        """n_iter solver iterations; wf, res, states updated in place."""
        self._step("hn_step", torch.float32, Medium(k_sq), wf, res, states, src, n_iter, res_hist, wf_hist, st_hist, rmse_hist)

    # ---- absorbing media: complex k_sq = k_sq + i k_sq_im (the hn_*_lossy entry points) ----
    def residual_lossy(self, wf: torch.Tensor, k_sq: torch.Tensor, k_sq_im: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
        """``residual`` with the complex pointwise term: L(wf) + (k_sq + i k_sq_im) wf - src; ``k_sq_im`` [B,1,h,w] fp32, any sign."""
        return self._residual(Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), wf, src)

    def step_lossy(self, wf, res, states, k_sq, k_sq_im, src, n_iter: int, res_hist=None, wf_hist=None, st_hist=None, rmse_hist=None):
        """``step`` on the lossy residual (hn_step_lossy): the same UNet launches, one lane, never a captured iteration."""
        self._step("hn_step", torch.float32, Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), wf, res, states, src, n_iter, res_hist, wf_hist, st_hist, rmse_hist)

    def fgmres_cycle_lossy(self, x: torch.Tensor, k_sq: torch.Tensor, k_sq_im: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float,
                           precond_iters: int, precond_scale: float, basis: Optional[torch.Tensor] = None, hess: Optional[torch.Tensor] = None,
                           zbasis: Optional[torch.Tensor] = None):
        """``fgmres_cycle`` on the lossy operator (hn_fgmres_cycle_lossy), preconditioned by ``precond_iters`` iterations of ``step_lossy``;
        ``precond_iters`` 0: plain restarted GMRES on the lossy operator.  Square domains.  Not capturable."""
        return self._fgmres_cycle("hn_fgmres_cycle", Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), x, rhs, restart, tol, precond_iters, precond_scale, basis,
                                  hess, zbasis)

    # ---- heterogeneous density: A_rho u = L(u) - b q . grad u + (k_sq [+ i k_sq_im]) u (the hn_*_medium entry points) ----
    def residual_medium(self, wf: torch.Tensor, k_sq: torch.Tensor, k_sq_im: Optional[torch.Tensor], rho_grad: torch.Tensor,
                        src: torch.Tensor) -> torch.Tensor:
        """``residual_lossy`` with the density term: ``rho_grad`` [B,2,h,w] fp32 holds d ln rho / dx (the last index) in plane 0 and d ln rho / dy in
        plane 1, per grid point (``helmnet_amd.density.log_density_gradient``).  ``k_sq_im`` may be None: a lossless medium."""
        return self._residual(Medium(k_sq, k_sq_im, _tensor(rho_grad, "rho_grad")), wf, src)

    def step_medium(self, wf, res, states, k_sq, k_sq_im, rho_grad, src, n_iter: int, res_hist=None, wf_hist=None, st_hist=None, rmse_hist=None):
        """``step_lossy`` on the variable-density residual (hn_step_medium); ``k_sq_im`` may be None."""
        self._step("hn_step", torch.float32, Medium(k_sq, k_sq_im, _tensor(rho_grad, "rho_grad")), wf, res, states, src, n_iter, res_hist, wf_hist, st_hist,
                   rmse_hist)

    def fgmres_cycle_medium(self, x: torch.Tensor, k_sq: torch.Tensor, k_sq_im: Optional[torch.Tensor], rho_grad: torch.Tensor, rhs: torch.Tensor,
                            restart: int, tol: float, precond_iters: int, precond_scale: float, basis: Optional[torch.Tensor] = None,
                            hess: Optional[torch.Tensor] = None, zbasis: Optional[torch.Tensor] = None):
        """``fgmres_cycle_lossy`` on the variable-density operator (hn_fgmres_cycle_medium), preconditioned by ``precond_iters`` iterations of
        ``step_medium``; ``precond_iters`` 0: plain restarted GMRES.  ``k_sq_im`` may be None.  Square domains.  Not capturable."""
        return self._fgmres_cycle("hn_fgmres_cycle", Medium(k_sq, k_sq_im, _tensor(rho_grad, "rho_grad")), x, rhs, restart, tol, precond_iters,
                                  precond_scale, basis, hess, zbasis)

    def residual64_lossy(self, wf: torch.Tensor, k_sq: torch.Tensor, k_sq_im: torch.Tensor, src: torch.Tensor, want_res: bool = True,
                         want_rmse: bool = True):
        """``residual64`` with the complex pointwise term (hn_residual_f64_lossy): (res [B,2,h,w] or None, rmse [B] or None), both float64, of
        L(wf) + (k_sq + i k_sq_im) wf - src.  Square and rectangular domains; always the float64 FFT route."""
        return self._residual64(Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), wf, src, want_res, want_rmse)

    def fgmres_refine_cycle_lossy(self, x: torch.Tensor, k_sq: torch.Tensor, k_sq_im: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float,
                                  precond_iters: int, precond_scale: float, inner_floor: float = 1e-6, basis: Optional[torch.Tensor] = None,
                                  hess: Optional[torch.Tensor] = None, zbasis: Optional[torch.Tensor] = None):
        """``fgmres_refine_cycle`` on the lossy operator (hn_fgmres_refine_cycle_lossy): the float64 residual of ``residual64_lossy``, the fp32 cycle of
        ``fgmres_cycle_lossy``, the preconditioner ``step_lossy``.  Returns (rmse64, rmse, k_used).  Square domains.  Not capturable."""
        return self._fgmres_refine_cycle(Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), x, rhs, restart, tol, precond_iters, precond_scale, inner_floor, basis,
                                         hess, zbasis)

    def residual_vjp_lossy(self, g: torch.Tensor, k_sq: torch.Tensor, k_sq_im: torch.Tensor) -> torch.Tensor:
        """A^H g of the lossy operator (hn_residual_vjp_lossy): L^H(g) + (k_sq - i k_sq_im) g, the J^T g of ``residual_lossy`` with respect to the
        wavefield.  Square and rectangular domains."""
        return self._residual_vjp(Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), g)

    def fgmres_adjoint_cycle_lossy(self, x: torch.Tensor, k_sq: torch.Tensor, k_sq_im: torch.Tensor, rhs: torch.Tensor, restart: int, tol: float,
                                   precond_iters: int, precond_scale: float, basis: Optional[torch.Tensor] = None,
                                   zbasis: Optional[torch.Tensor] = None, hess: Optional[torch.Tensor] = None):
        """``fgmres_adjoint_cycle`` on the lossy system A^H x = rhs (hn_fgmres_adjoint_cycle_lossy), A^H the operator of ``residual_vjp_lossy``,
        preconditioned by ``precond_iters`` iterations of ``step_lossy`` between the similarity weight.  Square domains.  Not capturable."""
        return self._fgmres_cycle("hn_fgmres_adjoint_cycle", Medium(k_sq, _tensor(k_sq_im, "k_sq_im")), x, rhs, restart, tol, precond_iters,
                                  precond_scale, basis, hess, zbasis)

    def adjoint_grad_lossy(self, lam: torch.Tensor, u: torch.Tensor, src_batch: Optional[int]):
        """``adjoint_grad`` for the lossy operator (hn_adjoint_grad_lossy): returns (g_k_sq, g_k_sq_im, g_src) with
        g_k_sq_im [B,1,n,n] = lam_re u_im - lam_im u_re; the other two as ``adjoint_grad`` returns them, bit for bit."""
        b = lam.shape[0]
        self._chk(lam, (b, 2, *self.hw), "lam")
        self._chk(u, (b, 2, *self.hw), "u")
        g_k_sq = torch.empty(b, 1, *self.hw, device=self.device, dtype=torch.float32)
        g_k_sq_im = torch.empty_like(g_k_sq)
        g_src = None if src_batch is None else torch.empty(int(src_batch), 2, *self.hw, device=self.device, dtype=torch.float32)
        rc = self.lib.hn_adjoint_grad_lossy(self.ctx, _ptr(lam), _ptr(u), 1 if src_batch is None else int(src_batch), b, _ptr(g_k_sq), _ptr(g_k_sq_im),
                                            _ptr(g_src), self._stream())
        _lib.check(rc, self.ctx, "hn_adjoint_grad_lossy")
        return g_k_sq, g_k_sq_im, g_src

    # ---- heterogeneous density: the adjoint operator and adjoint-state gradients ----
    def residual_vjp_medium(self, g: torch.Tensor, k_sq: torch.Tensor, k_sq_im: Optional[torch.Tensor], rho_grad: torch.Tensor) -> torch.Tensor:
        """A_rho^H g (hn_residual_vjp_medium): L^H g - D_x^H(conj(b_x) q_x g) - D_y^H(conj(b_y) q_y g) + (k_sq - i k_sq_im) g, the J^T g of
        ``residual_medium`` with respect to the wavefield.  ``k_sq_im`` may be None.  Square and rectangular domains."""
        return self._residual_vjp(Medium(k_sq, k_sq_im, _tensor(rho_grad, "rho_grad")), g)

    def fgmres_adjoint_cycle_medium(self, x: torch.Tensor, k_sq: torch.Tensor, k_sq_im: Optional[torch.Tensor], rho_grad: torch.Tensor,
                                    rho: Optional[torch.Tensor], rhs: torch.Tensor, restart: int, tol: float, precond_iters: int, precond_scale: float,
                                    basis: Optional[torch.Tensor] = None, zbasis: Optional[torch.Tensor] = None, hess: Optional[torch.Tensor] = None):
        """``fgmres_adjoint_cycle_lossy`` on A_rho^H x = rhs (hn_fgmres_adjoint_cycle_medium), preconditioned by ``precond_iters`` iterations of
        ``step_medium`` between the similarity weight W / rho: ``rho`` [B,1,n,n] fp32, positive (only its ratios matter); None is allowed with
        ``precond_iters`` 0 alone, which is plain restarted GMRES on A_rho^H.  ``k_sq_im`` may be None.  Square domains.  Not capturable."""
        return self._fgmres_cycle("hn_fgmres_adjoint_cycle", Medium(k_sq, k_sq_im, _tensor(rho_grad, "rho_grad")), x, rhs, restart, tol, precond_iters,
                                  precond_scale, basis, hess, zbasis, rho=(rho,))

    def adjoint_grad_medium(self, lam: torch.Tensor, u: torch.Tensor, src_batch: Optional[int], lossy: bool = True):
        """``adjoint_grad_lossy`` for the variable-density operator (hn_adjoint_grad_medium): returns (g_k_sq, g_k_sq_im, g_rho_grad, g_src) with
        g_rho_grad [B,2,n,n] = dJ/dq: plane 0 Re(conj(lam) b_x D_x u), plane 1 Re(conj(lam) b_y D_y u); the others as ``adjoint_grad_lossy`` returns
        them, bit for bit.  ``lossy`` False (a medium without absorption): g_k_sq_im is None and is not computed."""
        b = lam.shape[0]
        self._chk(lam, (b, 2, *self.hw), "lam")
        self._chk(u, (b, 2, *self.hw), "u")
        g_k_sq = torch.empty(b, 1, *self.hw, device=self.device, dtype=torch.float32)
        g_k_sq_im = torch.empty_like(g_k_sq) if lossy else None
        g_rho_grad = torch.empty(b, 2, *self.hw, device=self.device, dtype=torch.float32)
        g_src = None if src_batch is None else torch.empty(int(src_batch), 2, *self.hw, device=self.device, dtype=torch.float32)
        rc = self.lib.hn_adjoint_grad_medium(self.ctx, _ptr(lam), _ptr(u), 1 if src_batch is None else int(src_batch), b, _ptr(g_k_sq), _ptr(g_k_sq_im),
                                             _ptr(g_rho_grad), _ptr(g_src), self._stream())
        _lib.check(rc, self.ctx, "hn_adjoint_grad_medium")
        return g_k_sq, g_k_sq_im, g_rho_grad, g_src

    # ---- training step (hn_train_grad / hn_adam_step) -------------------------------------------------
    def train_reserve(self, batch: int, n_unroll: int):
        _lib.check(self.lib.hn_train_reserve(self.ctx, int(batch), int(n_unroll)), self.ctx, "hn_train_reserve")

    def train_grad(self, weights, wf, res, states, k_sq, src, n_unroll: int, loss_scale: float = 1e4, input_grads: bool = False,
                   grad: Optional[torch.Tensor] = None) -> dict:
        """Loss and gradients of ``n_unroll`` unrolled solver iterations (hybridnet.py:399-409).  ``weights``: flat device blob
        (pack_weights order).  Returns loss [1], grad (same shape as weights), the wavefield / residual / state lists of
        ``n_steps(..., True, True)`` as stacked tensors, and with ``input_grads`` the gradients of the three inputs."""
        b, n_w = wf.shape[0], int(self.lib.hn_weight_count(8, self.depth, 2))
        self._chk(weights, (n_w,), "weights")
        self._chk(wf, (b, 2, *self.hw), "wavefield")
        self._chk(res, (b, 2, *self.hw), "residual")
        self._chk(states, (b, 2, self.state_len), "hidden state")
        self._chk(k_sq, (b, 1, *self.hw), "k_sq")
        self._chk(src, (src.shape[0], 2, *self.hw), "source")
        T = int(n_unroll)
        new = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)  # noqa: E731
        out = {"wavefields": new(T, b, 2, *self.hw), "residuals": new(T, b, 2, *self.hw), "states": new(T, b, 2, self.state_len),
               "loss": new(1), "grad": grad if grad is not None else new(n_w)}
        self._chk(out["grad"], (n_w,), "grad")
        g_in = [new(*wf.shape), new(*res.shape), new(*states.shape)] if input_grads else [None, None, None]
        rc = self.lib.hn_train_grad(self.ctx, _ptr(weights), _ptr(wf), _ptr(res), _ptr(states), _ptr(k_sq), _ptr(src), src.shape[0], b, T,
                                    float(loss_scale), _ptr(out["wavefields"]), _ptr(out["residuals"]), _ptr(out["states"]), _ptr(out["loss"]),
                                    _ptr(out["grad"]), _ptr(g_in[0]), _ptr(g_in[1]), _ptr(g_in[2]), self._stream())
        _lib.check(rc, self.ctx, "hn_train_grad")
        if input_grads:
            out.update(grad_wf=g_in[0], grad_res=g_in[1], grad_states=g_in[2])
        return out

    def step_vjp(self, weights, wf0, res0, states0, k_sq, src_batch: int, wf_hist, res_hist, st_hist, g_wf_hist=None, g_res_hist=None,
                 g_st_hist=None, g_wf_T=None, g_res_T=None, g_st_T=None, g_k_sq=None, g_src=None, g_weights=None, flags: int = 0) -> dict:
        """hn_step_vjp: reverse mode of ``n_iter = wf_hist.shape[0]`` solver iterations, the histories of ``step`` being the tape.  Returns the
        gradients with respect to wf0 / res0 / states0 (new tensors); ``g_k_sq`` [B,1,n,n], ``g_src`` [src_batch,2,n,n] and ``g_weights`` are
        accumulated into when given.  ``flags``: sum of _lib.HN_VJP values (segments of one long solve, see the header)."""
        b, T = wf0.shape[0], int(wf_hist.shape[0])
        n_w = int(self.lib.hn_weight_count(8, self.depth, 2))
        self._chk(weights, (n_w,), "weights")
        for t, shape, name in ((wf0, (b, 2, *self.hw), "wavefield"), (res0, (b, 2, *self.hw), "residual"),
                               (states0, (b, 2, self.state_len), "hidden state"), (k_sq, (b, 1, *self.hw), "k_sq"),
                               (wf_hist, (T, b, 2, *self.hw), "wf_hist"), (res_hist, (T, b, 2, *self.hw), "res_hist"),
                               (st_hist, (T, b, 2, self.state_len), "st_hist")):
            self._chk(t, shape, name)
        for t, shape, name in ((g_wf_hist, wf_hist.shape, "g_wf_hist"), (g_res_hist, res_hist.shape, "g_res_hist"), (g_st_hist, st_hist.shape, "g_st_hist"),
                               (g_wf_T, wf0.shape, "g_wf_T"), (g_res_T, res0.shape, "g_res_T"), (g_st_T, states0.shape, "g_st_T"),
                               (g_k_sq, k_sq.shape, "g_k_sq"), (g_src, (int(src_batch), 2, *self.hw), "g_src"), (g_weights, (n_w,), "g_weights")):
            if t is not None:
                self._chk(t, shape, name)
        out = {"grad_wf": torch.empty_like(wf0), "grad_res": torch.empty_like(res0), "grad_states": torch.empty_like(states0)}
        rc = self.lib.hn_step_vjp(self.ctx, _ptr(weights), _ptr(wf0), _ptr(res0), _ptr(states0), _ptr(k_sq), int(src_batch), b, T,
                                  _ptr(wf_hist), _ptr(res_hist), _ptr(st_hist), _ptr(g_wf_hist), _ptr(g_res_hist), _ptr(g_st_hist),
                                  _ptr(g_wf_T), _ptr(g_res_T), _ptr(g_st_T), _ptr(out["grad_wf"]), _ptr(out["grad_res"]), _ptr(out["grad_states"]),
                                  _ptr(g_k_sq), _ptr(g_src), _ptr(g_weights), int(flags), self._stream())
        _lib.check(rc, self.ctx, "hn_step_vjp")
        return out

    def step_jvp(self, wf0, res0, states0, k_sq, src_batch: int, wf_hist, res_hist, st_hist, t_wf, t_res, t_states, t_k_sq=None, t_src=None,
                 t_wf_hist=None, t_res_hist=None, t_st_hist=None) -> dict:
        """hn_step_jvp: forward mode of ``n_iter = wf_hist.shape[0]`` solver iterations, the histories of ``step`` being the tape.  ``t_wf`` /
        ``t_res`` / ``t_states`` hold the tangents of (wf0, res0, states0) and are updated IN PLACE to those of the last iteration's outputs
        (the same three tensors are returned); ``t_k_sq`` [B,1,n,n] and ``t_src`` [src_batch,2,n,n] are the
        directions on k_sq and the source (None = zero); the optional histories receive the tangents after every iteration."""
        b, T = wf0.shape[0], int(wf_hist.shape[0])
        for t, shape, name in ((wf0, (b, 2, *self.hw), "wavefield"), (res0, (b, 2, *self.hw), "residual"),
                               (states0, (b, 2, self.state_len), "hidden state"), (k_sq, (b, 1, *self.hw), "k_sq"),
                               (wf_hist, (T, b, 2, *self.hw), "wf_hist"), (res_hist, (T, b, 2, *self.hw), "res_hist"),
                               (st_hist, (T, b, 2, self.state_len), "st_hist"), (t_wf, wf0.shape, "t_wf"), (t_res, res0.shape, "t_res"),
                               (t_states, states0.shape, "t_states")):
            self._chk(t, shape, name)
        for t, shape, name in ((t_k_sq, k_sq.shape, "t_k_sq"), (t_src, (int(src_batch), 2, *self.hw), "t_src"),
                               (t_wf_hist, wf_hist.shape, "t_wf_hist"), (t_res_hist, res_hist.shape, "t_res_hist"), (t_st_hist, st_hist.shape, "t_st_hist")):
            if t is not None:
                self._chk(t, shape, name)
        rc = self.lib.hn_step_jvp(self.ctx, _ptr(wf0), _ptr(res0), _ptr(states0), _ptr(k_sq), int(src_batch), b, T, _ptr(wf_hist), _ptr(res_hist),
                                  _ptr(st_hist), _ptr(t_wf), _ptr(t_res), _ptr(t_states), _ptr(t_k_sq), _ptr(t_src), _ptr(t_wf_hist), _ptr(t_res_hist),
                                  _ptr(t_st_hist), self._stream())
        _lib.check(rc, self.ctx, "hn_step_jvp")
        return {"t_wf": t_wf, "t_res": t_res, "t_states": t_states}

    def adam_step(self, weights, grad, exp_avg, exp_avg_sq, step: int, lr: float, betas=(0.9, 0.95), eps: float = 1e-8,
                  weight_decay: float = 0.0, clip_value: float = 0.0, trainable: Optional[torch.Tensor] = None):
        """clip_grad_value_ + torch.optim.Adam step (hybridnet.py:172-176, 250-258) on caller-owned flat device tensors, in place."""
        n = weights.numel()
        for t, name in ((weights, "weights"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            self._chk(t, (n,), name)
        if trainable is not None and (trainable.dtype != torch.uint8 or trainable.numel() != n or trainable.device != self.device):
            raise ValueError("trainable must be a uint8 device tensor with one entry per weight")
        rc = self.lib.hn_adam_step(self.ctx, _ptr(weights), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(trainable), n, float(lr),
                                   float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(clip_value), int(step), self._stream())
        _lib.check(rc, self.ctx, "hn_adam_step")

    # ---- rows of a replay buffer (hn_rows_gather / hn_rows_scatter) ----------------------------------------------------
    def _rows_args(self, buffers, slots):
        n = len(buffers)
        cap = buffers[0].shape[0]
        for b in buffers:
            if b.dtype != torch.float32 or b.device != self.device or not b.is_contiguous() or b.shape[0] != cap:
                raise ValueError("replay-buffer fields must be contiguous fp32 [capacity, ...] tensors on the engine's device")
        slots = np.ascontiguousarray(np.asarray(slots).reshape(-1), dtype=np.int32)
        rows = (ctypes.c_int64 * n)(*[b[0].numel() for b in buffers])
        return n, cap, slots, rows, (ctypes.c_void_p * n)(*[b.data_ptr() for b in buffers])

    def rows_gather(self, buffers, slots):
        """ReplayBuffer.sample's stack (replaybuffer.py:37-47): [len(slots), ...] copies of rows ``slots`` (host integers) of every buffer, one launch."""
        n, cap, slots, rows, bufs = self._rows_args(buffers, slots)
        out = [torch.empty((slots.size,) + tuple(b.shape[1:]), dtype=torch.float32, device=self.device) for b in buffers]
        outs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in out])
        rc = self.lib.hn_rows_gather(self.ctx, n, bufs, rows, cap, slots.ctypes.data_as(ctypes.c_void_p), int(slots.size), outs, self._stream())
        _lib.check(rc, self.ctx, "hn_rows_gather")
        return out

    def rows_scatter(self, buffers, slots, new_rows):
        """ReplayBuffer.append for a batch of slots (replaybuffer.py:29-30): ``buffers[f][slots[j]] = new_rows[f][j]``; ``None`` writes zeros, a tensor
        with ONE row is written to every slot.  One launch."""
        n, cap, slots, rows, bufs = self._rows_args(buffers, slots)
        keep, ptrs, strides = [], [], []
        for b, v in zip(buffers, new_rows):
            if v is None:
                ptrs.append(None); strides.append(0)
                continue
            if v.dtype != torch.float32 or v.device != self.device or tuple(v.shape[1:]) != tuple(b.shape[1:]) or v.shape[0] not in (1, slots.size):
                raise ValueError(f"new rows of shape {tuple(v.shape)} do not fit {slots.size} slots of {tuple(b.shape[1:])}")
            v = v.contiguous()
            keep.append(v)
            ptrs.append(v.data_ptr()); strides.append(0 if (v.shape[0] == 1 and slots.size > 1) else b[0].numel())
        rc = self.lib.hn_rows_scatter(self.ctx, n, bufs, rows, cap, slots.ctypes.data_as(ctypes.c_void_p), int(slots.size),
                                      (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int64 * n)(*strides), self._stream())
        _lib.check(rc, self.ctx, "hn_rows_scatter")

    # ---- a stream of maps solved to a tolerance (hn_stream_verdict / hn_stream_swap) ------------------------------------
    VERDICT_DTYPE = np.dtype([("first_below", np.int32), ("bad", np.int32), ("last_rmse", np.float32)])   # struct hn_stream_verdict_rec

    def stream_verdict(self, rmse_hist: torch.Tensor, tol: float, diverge_rmse: Optional[float] = None) -> np.ndarray:
        """One launch over the [n_rows, batch] RMSE rows a chunk of ``step`` wrote.  Returns a VIEW (no copy) of the context's pinned table as a
        structured array of ``batch`` records (first_below, bad, last_rmse): valid once the current stream has been synchronised and until the
        next call.  ``diverge_rmse`` None: only NaN / Inf rows mark a slot as bad."""
        n_rows, b = int(rmse_hist.shape[0]), int(rmse_hist.shape[1])
        self._chk(rmse_hist, (n_rows, b), "rmse_hist")
        table = ctypes.c_void_p()
        rc = self.lib.hn_stream_verdict(self.ctx, _ptr(rmse_hist), n_rows, b, float(tol), float("inf") if diverge_rmse is None else float(diverge_rmse),
                                        ctypes.byref(table), self._stream())
        _lib.check(rc, self.ctx, "hn_stream_verdict")
        raw = (ctypes.c_char * (self.VERDICT_DTYPE.itemsize * b)).from_address(table.value)
        return np.frombuffer(raw, dtype=self.VERDICT_DTYPE, count=b)

    def stream_swap(self, wf, res, states, k_sq, src, ops, sos_in=None, src_in=None, omega: float = 1.0, out_wf=None, out_res=None):
        """Retire / move / refill slots of the batch arrays in one launch (hn_stream_swap).  ``ops``: rows of (slot, retire_map, move_from,
        refill_map), -1 = none -- host integers, they travel in the kernel arguments.  ``sos_in`` [n_maps,1,n,n] / ``src_in`` [n_maps,2,n,n]
        feed refills (``src_in`` only when ``src`` has one row per slot), ``out_wf`` / ``out_res`` [n_maps,2,n,n] receive retired slots."""
        b = wf.shape[0]
        self._chk(wf, (b, 2, *self.hw), "wavefield")
        self._chk(res, (b, 2, *self.hw), "residual")
        self._chk(states, (b, 2, self.state_len), "hidden state")
        self._chk(k_sq, (b, 1, *self.hw), "k_sq")
        self._chk(src, (src.shape[0], 2, *self.hw), "source")
        n_maps = {int(t.shape[0]) for t in (sos_in, src_in, out_wf, out_res) if t is not None}
        if len(n_maps) > 1:
            raise ValueError(f"sos_in / src_in / out_wf / out_res disagree on the number of maps: {sorted(n_maps)}")
        n_maps = n_maps.pop() if n_maps else 0
        for t, ch, name in ((sos_in, 1, "sos_in"), (src_in, 2, "src_in"), (out_wf, 2, "out_wf"), (out_res, 2, "out_res")):
            if t is not None:
                self._chk(t, (n_maps, ch, *self.hw), name)
        ops = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1, 4))
        rc = self.lib.hn_stream_swap(self.ctx, _ptr(wf), _ptr(res), _ptr(states), _ptr(k_sq), _ptr(src), int(src.shape[0]), b, int(ops.shape[0]),
                                     ops.ctypes.data_as(ctypes.c_void_p), _ptr(sos_in), _ptr(src_in), n_maps, float(omega), _ptr(out_wf), _ptr(out_res),
                                     self._stream())
        _lib.check(rc, self.ctx, "hn_stream_swap")

    def set_train_forward_event(self, event: Optional[torch.cuda.Event], sumsq_host: Optional[torch.Tensor] = None) -> None:
        """hn_train_set_forward_event: ``event`` is recorded behind the forward sweep of every later ``train_grad`` (None clears it); ``sumsq_host``
        (a pinned fp32 host tensor) receives the [n_unroll, batch] table of per-sample sums of res^2 before the event fires."""
        handle, table, cap = None, None, 0
        if event is not None:
            if not event.cuda_event:      # (torch creates the HIP event lazily: recording it once makes the handle exist)
                event.record(torch.cuda.current_stream(self.device))
            handle = ctypes.c_void_p(event.cuda_event)
        if sumsq_host is not None:
            if sumsq_host.dtype != torch.float32 or sumsq_host.device.type != "cpu" or not sumsq_host.is_pinned() or not sumsq_host.is_contiguous():
                raise ValueError("sumsq_host must be a contiguous pinned fp32 host tensor")
            table, cap = ctypes.c_void_p(sumsq_host.data_ptr()), sumsq_host.numel()
        _lib.check(self.lib.hn_train_set_forward_event(self.ctx, handle, table, cap), self.ctx, "hn_train_set_forward_event")
        self._fwd_event, self._fwd_sumsq = event, sumsq_host           # keep them alive while the library holds the handles

    PEEK = {"x": 0, "sig_mid": 1, "out": 2, "st_mid": 3, "u": 4, "dec_mid": 5, "y": 6, "inc_mid": 7, "g_x": 16, "g_out": 18, "g_u": 20, "g_y": 22}

    def train_peek(self, kind: str, level: int, batch: int) -> torch.Tensor:
        """Debug / test aid: one tape tensor or activation gradient of iteration 0 of the last train_grad call."""
        ch = 2 if kind == "st_mid" else 8
        m = self.n >> level
        out = torch.empty(batch, ch, m, m, device=self.device, dtype=torch.float32)
        got = self.lib.hn_train_peek(self.ctx, self.PEEK[kind], int(level), _ptr(out), out.numel(), self._stream())
        if got < 0:
            _lib.check(int(got), self.ctx, "hn_train_peek")
        return out

    # ---- measurement hooks ---------------------------------------------------------------
    KERNEL_IDS = 37

    @staticmethod
    def kernel_name(kid: int) -> str:
        if kid == 0:
            return "inc"
        if 1 <= kid <= 18:
            return ("conv_signal", "conv_state", "down")[(kid - 1) % 3] + str((kid - 1) // 3)
        if kid == 19:
            return "bottleneck"
        if 20 <= kid <= 31:
            return ("up", "decode")[(kid - 20) % 2] + str((kid - 20) // 2)
        return {32: "spectral_cols", 33: "spectral_rows", 34: "deep", 35: "spectral_pair", 36: "inc_conv_signal0"}[kid]

    def profile_enable(self, kernel_ids=None):
        """Bracket the selected kernels (None = all, [] = none) with HIP events on the launch stream."""
        mask = (1 << self.KERNEL_IDS) - 1 if kernel_ids is None else sum(1 << k for k in kernel_ids)
        _lib.check(self.lib.hn_profile_enable(self.ctx, ctypes.c_uint64(mask)), self.ctx, "hn_profile_enable")

    def profile_min(self) -> dict:
        """{kernel name: shortest bracketed launch in ms} for the interval closed by the last profile_collect()."""
        ms = (ctypes.c_double * self.KERNEL_IDS)()
        _lib.check(self.lib.hn_profile_min(self.ctx, ms, self.KERNEL_IDS), self.ctx, "hn_profile_min")
        return {self.kernel_name(i): ms[i] for i in range(self.KERNEL_IDS) if ms[i] > 0}

    def profile_stride(self, every_nth: int):
        """Bracket only every n-th launch of the selected kernels (an event pair costs microseconds of gap)."""
        _lib.check(self.lib.hn_profile_stride(self.ctx, int(every_nth)), self.ctx, "hn_profile_stride")

    def profile_collect(self) -> dict:
        """{kernel name: (total ms, launches)} since the last collect."""
        ms = (ctypes.c_double * self.KERNEL_IDS)()
        cnt = (ctypes.c_int64 * self.KERNEL_IDS)()
        _lib.check(self.lib.hn_profile_collect(self.ctx, ms, cnt, self.KERNEL_IDS), self.ctx, "hn_profile_collect")
        return {self.kernel_name(i): (ms[i], int(cnt[i])) for i in range(self.KERNEL_IDS) if cnt[i]}
