"""Seeded fresh weights for networks other than the shipped checkpoint (any depth, activation, ``state_depth`` and PReLU slope plan).

Shared by ``tests/golden/make_golden_configs.py`` (which runs the reference on them) and the tests, so both build the same tensors from
the seed: ``numpy.random.default_rng`` (PCG64) streams are stable across numpy releases, torch's generator is not part of that promise.

Each convolution is scaled by gain / sqrt(fan_in).  The gain undoes the RMS change of the activation in front of it (a PReLU with slope a
maps a symmetric input of RMS r to RMS r * sqrt((1 + a^2) / 2)); the 8x8 convolutions of levels 8 / 4 / 2 wide get 1.6 / 2.2 / 2.5, and the
DoubleConvs of levels 2 / 1 wide the square roots of 1.6 / 2.2, because the padding of the convolutions eats taps there (so the weights
depend on the domain size ``n`` they are made for).  Plain N(0, 0.3) weights reach 1e17 at depth 6; ``tape_check`` states what these keep, and
tests/test_config_weights.py runs it on every configuration the fixture and the GPU tests use.

Slope plans (every PReLU layer in blob order; ``engine.weight_names``):
  A  alternates 3.0, -0.4, 1.6, -0.4 -- every layer has a slope above 1 or a negative one
  B  swaps them: a slope above 1 becomes -0.4, a negative one 3.0 / 1.6
Across the two plans every layer, and so every kernel family (inc, conv_signal_0, conv_state_0 / _1, decode_0, the level-1 layers, the
deep levels, the bottleneck), runs both the slope > 1 branch and the negative-slope branch of its epilogue, wherever ``tape_check`` finds
enough negative pre-activations.  The slopes 0 and 0.01 are the constant ones of relu / leakyrelu; the shipped checkpoint's lie in
[-0.30, 0.76].
"""
from typing import Dict, Optional

import numpy as np

from helmnet_amd.engine import weight_shapes

_PLAN_A = (3.0, -0.4, 1.6, -0.4)
_SWAP = {3.0: -0.4, 1.6: -0.4}


def slope_plan(plan: str, n_layers: int) -> list:
    """The slope of each of ``n_layers`` PReLU layers (blob order) under plan 'A' or 'B'."""
    a = [_PLAN_A[i % 4] for i in range(n_layers)]
    if plan == "A":
        return a
    if plan == "B":
        return [_SWAP[s] if s > 1 else (3.0 if i % 4 == 1 else 1.6) for i, s in enumerate(a)]
    raise KeyError(plan)


# extra gain of an 8x8 convolution on a level this wide (its padding eats taps) and of a 3x3 one at a quarter of that width
_NARROW_GAIN = {8: 1.6, 4: 2.2, 2: 2.5}


def _fan_in(name: str, shape) -> int:
    if name.startswith("up."):          # ConvTranspose2d [cin, cout, 8, 8], stride 2: each output sees cin * 4 * 4 taps
        return shape[0] * 16
    return int(np.prod(shape[1:]))


def config_weights(depth: int, seed: int, slopes: Optional[str] = "A", act: str = "prelu", state_depth: Optional[int] = None,
                   n: int = 64) -> Dict[str, np.ndarray]:
    """A HybridNet state dict (float32 arrays, reference names and shapes) for ``depth`` 1..6, scaled for an n^2 domain.

    ``slopes``: plan 'A' / 'B' for prelu (ignored otherwise: the parameter-free activations have no ``double_conv.1.weight``).
    ``state_depth < depth``: levels d >= state_depth are built as the reference builds them (architectures.py:202-218): conv_signal sees
    the 8 features only and there is no conv_state."""
    state_depth = depth if state_depth is None else state_depth
    shapes = weight_shapes(depth)
    rng = np.random.default_rng(seed)
    prelu_names = [k for k in shapes if k.endswith(".double_conv.1.weight")]
    plan = dict(zip(prelu_names, slope_plan(slopes, len(prelu_names)))) if act == "prelu" else {}
    out = {}
    for name, shape in shapes.items():
        level = name.split(".")[1] if name.startswith("enc.") else None
        stateless = level is not None and int(level) >= state_depth
        if stateless and ".conv_state." in name:
            continue
        if stateless and name.endswith(".conv_signal.double_conv.0.weight"):
            shape = (shape[0], 8) + tuple(shape[2:])
        if name.endswith(".double_conv.1.weight"):
            if act == "prelu":
                out[name] = np.full(shape, plan[name], np.float32)
            continue
        if name.endswith("bias"):
            out[name] = (0.05 * rng.standard_normal(shape)).astype(np.float32)
            continue
        gain = 1.0
        if ".down." in name or name.startswith("up."):
            gain = _NARROW_GAIN.get(n >> int(name.split(".")[1]), 1.0)
        if name.endswith(".double_conv.2.weight"):    # behind the activation: undo its RMS change
            a = plan.get(name.replace("2.weight", "1.weight"), 0.0 if act in ("prelu", "relu") else 0.5)
            gain = float(np.sqrt(2.0 / (1.0 + a * a)))
        if name.startswith("decode.") and ".double_conv." in name:
            gain *= _NARROW_GAIN.get(4 * (n >> int(name.split(".")[1])), 1.0) ** 0.5   # 3x3 convolutions on maps 2 wide or less
        out[name] = (gain / np.sqrt(_fan_in(name, shape)) * rng.standard_normal(shape)).astype(np.float32)
    return out


def config_input(n: int, b: int, depth: int, seed: int, wf_scale: float = 0.5):
    """Seeded network input x6 = [wf, 1e3 * res, sigma_x, sigma_y] at n^2 (the sigmas of the 8-point PML the solver uses) and a flat
    hidden state for ``depth`` levels: float32 arrays."""
    from oracle import helmnet_oracle as O
    rng = np.random.default_rng(seed)
    f32 = np.float32
    wf = (wf_scale * rng.standard_normal((b, 2, n, n))).astype(f32)
    res = (5e-3 * rng.standard_normal((b, 2, n, n))).astype(f32)
    L = sum((n >> d) ** 2 for d in range(depth))
    states = (0.5 * rng.standard_normal((b, 2, L))).astype(f32)
    sos = (1.0 + rng.random((b, 1, n, n))).astype(f32)
    sig = O.SpectralTables(n, 8, 2, 1.0).sigmas.numpy()
    x6 = np.concatenate([wf, (1e3 * res.astype(np.float64)).astype(f32), np.broadcast_to(sig, (b, 2, n, n))], 1).astype(f32)
    return {"wf": wf, "res": res, "states": states, "sos": sos, "x6": np.ascontiguousarray(x6)}


def tape_check(tape: dict):
    """On an oracle tape (``O.unet_forward(..., tape=...)``): the first convolution of every DoubleConv has at least 20 % negative
    pre-activations (so the slope branch of every layer's epilogue is used), and every recorded tensor's RMS lies in [0.1, 10]."""
    neg = {k: float((v < 0).double().mean()) for k, v in tape.items() if k.endswith(".mid")}
    rms = {k: float(v.double().pow(2).mean().sqrt()) for k, v in tape.items() if not k.startswith("__")}
    low = {k: v for k, v in neg.items() if v < 0.2}
    off = {k: v for k, v in rms.items() if not 0.1 <= v <= 10}
    assert not low and not off, (low, off)


# the configurations of tests/golden/configs.npz (64^2, batch 1, input seed GOLDEN_INPUT_SEED): tag -> (depth, seed, slope plan, activation,
# state_depth).  Seeds picked so that tape_check holds (tests/test_config_weights.py).
GOLDEN_CONFIGS = {
    "d1A": (1, 701, "A", "prelu", 1), "d1B": (1, 701, "B", "prelu", 1),
    "d2A": (2, 702, "A", "prelu", 2), "d2B": (2, 702, "B", "prelu", 2),
    "d3A": (3, 701, "A", "prelu", 3), "d3B": (3, 703, "B", "prelu", 3),
    "d5A": (5, 705, "A", "prelu", 5), "d5B": (5, 705, "B", "prelu", 5),
    "d6A": (6, 706, "A", "prelu", 6), "d6B": (6, 704, "B", "prelu", 6),
    "d3relu": (3, 703, None, "relu", 3), "d3softplus": (3, 703, None, "softplus", 3),
    "d5sd2": (5, 705, "A", "prelu", 2),
}
GOLDEN_N, GOLDEN_B, GOLDEN_INPUT_SEED = 64, 1, 4545

# the teacher-forced configurations of tests/test_config_matrix.py: tag -> (depth, seed, slope plan, activation, state_depth, n, batch); the
# input seed is 9000 + n, the teacher wavefield 1e-6 (see there)
GPU_CONFIGS = {
    "d4_256_A": (4, 741, "A", "prelu", 4, 256, 3), "d4_256_B": (4, 741, "B", "prelu", 4, 256, 3),
    "d4_256_relu": (4, 741, None, "relu", 4, 256, 3), "d4_256_leakyrelu": (4, 741, None, "leakyrelu", 4, 256, 3),
    "d4_512_A": (4, 742, "A", "prelu", 4, 512, 1), "d4_512_B": (4, 742, "B", "prelu", 4, 512, 1),
    "d4_256_A_b33": (4, 741, "A", "prelu", 4, 256, 33),
    "d3_128": (3, 751, "A", "prelu", 3, 128, 5), "d3_256": (3, 743, "B", "prelu", 3, 256, 2),
    "d2_128": (2, 744, "A", "prelu", 2, 128, 2), "d2_64": (2, 744, "B", "prelu", 2, 64, 3),
    "d5_512": (5, 751, "A", "prelu", 5, 512, 1), "d6_256": (6, 746, "B", "prelu", 6, 256, 2), "d1_256": (1, 747, "A", "prelu", 1, 256, 2),
    "d4_256_sd2": (4, 748, "B", "prelu", 2, 256, 3), "d4_512_sd0": (4, 748, "A", "prelu", 0, 512, 1),
    "d4_256_softplus": (4, 741, None, "softplus", 4, 256, 2), "d4_256_gelu": (4, 741, None, "gelu", 4, 256, 2),
    "d4_512_softplus": (4, 742, None, "softplus", 4, 512, 1), "d4_512_gelu": (4, 742, None, "gelu", 4, 512, 1),
    "d4_272_A": (4, 749, "A", "prelu", 4, 272, 3), "d4_512_A16": (4, 742, "A", "prelu", 4, 512, 1),
    "d4_528_A": (4, 742, "A", "prelu", 4, 528, 1),      # 528 = 16 * 33: level 3 is 66 wide, the bottleneck 33 (odd and wider than 32)
}

# the training / reverse-mode configurations of tests/train_matrix.py (test_train_matrix_gpu.py, test_train_matrix_host.py): tag -> (depth,
# seed, slope plan, activation, state_depth, n, batch); the input seed is 7000 + n (train_matrix.train_case).  Seeds picked so that
# tape_check holds (tests/test_config_weights.py).  528 = 16 * 33: the only way to an odd level wider than 32 is an odd bottleneck
TRAIN_CONFIGS = {
    "d4_528": (4, 760, "A", "prelu", 4, 528, 1),
    "d4_80_A": (4, 760, "A", "prelu", 4, 80, 2), "d4_80_B": (4, 760, "B", "prelu", 4, 80, 2),
    "d1_80": (1, 760, "A", "prelu", 1, 80, 2), "d2_112": (2, 760, "B", "prelu", 2, 112, 1), "d3_144": (3, 760, "B", "prelu", 3, 144, 1),
    "d5_96": (5, 760, "A", "prelu", 5, 96, 2), "d6_192": (6, 760, "B", "prelu", 6, 192, 1), "d6_64": (6, 781, "A", "prelu", 6, 64, 2),
    "d5_160_sd2": (5, 760, "A", "prelu", 2, 160, 1), "d4_64_sd0": (4, 760, "B", "prelu", 0, 64, 2),
    "d4_80_relu": (4, 760, None, "relu", 4, 80, 2), "d4_64_tanhshrink": (4, 769, None, "tanhshrink", 4, 64, 1),
    "d4_64_gelu": (4, 760, None, "gelu", 4, 64, 2), "d5_96_tanh": (5, 760, None, "tanh", 5, 96, 2),
    "d4_160_A": (4, 760, "A", "prelu", 4, 160, 1),      # level 0 at least 128 wide: the fused forward kernel is the strip kernel there
}
TRAIN_INPUT_SEED = 7000
