"""Cases and float64 references for the layer-level tests of the network's own DoubleConv / 8x8 dispatch (launch_dc8, launch_down, launch_up: the
matrix-core kernels of hn_mfma.hip, hn_dcv.hip and hn_dca.hip), driven one layer at a time through hn_double_conv / hn_conv8x8 with the option
'module_mc' (HN_OPT_MODULE_MC).  TEST CODE ONLY; used by tests/test_mc_layers_host.py (CPU) and tests/test_mc_layers_gpu.py.

TABLE names, per kernel instance (enum hn_route of include/helmnet_hip.h), the planes at which it can go wrong -- one tile, one tile plus a row and a column
(two columns where the route needs an even W), two tiles and a part both ways with H != W, where the instance's width range has room for them -- and the
settings (precision mode, 'mc_stage', 'dc_valu') under which hn_module_route must name that instance for them.  Tile sizes as the kernels have them:
strips 16 x 64 (k_dc_x16 in bf16x3: 8 x 64), k_dc_mfma_p 8 x 32 / 8 x 16, k_dc_mfma 16 x 64 / 32 / 16, hn_dcv.hip / hn_dca.hip 16 x 64, down 16 rows x
64 / 32 / 16 OUTPUTS (k_down_x16: 16 x 16), up 22 window rows x 32 INPUT columns above 64 columns, 20 x 16 at and below and in k_up_x16 (window rows
-1 .. Hin - 1: the first block ends with input row 20 / 18).

References are plain F.conv2d / F.conv_transpose2d compositions in float64.

EXACT legs.  Inputs, weights and biases are small signed integers and the PReLU slope is 2, -0.5, 0.25 or 0 (relu), so every product, every partial sum in
any order and every stored mid value is exactly representable in fp32, in fp16 (11 significant bits: integers to 2048, multiples of 1/4 to 512) and in
the 2- and 3-part bf16 splits (16 / 24 bits; the 2-part mode drops the product of the two SECOND parts, which is zero whenever one operand fits 8 bits:
|integer| <= 256 -- every product below has such an operand): a correct kernel in any precision mode returns the float64 reference bit for bit.
    DoubleConv  x, w1, w2 in [-2, 2], biases in [-3, 3]      reference at 35 x 194 x 2: max |mid| 226, max |out| 1978
    8x8         x, w in [-4, 4], bias in [-3, 3]             reference max |out| 618 (down, 38 x 134), 341 (up, 23 x 67)
tests/test_mc_layers_host.py asserts the preconditions on the reference of every case: 4 * mid an integer with |mid| <= 512, |out| < 2^24, inputs
integers of magnitude <= 4.
IMPULSE cases: sample s holds a single 1, in channel s, at one of three positions (an image corner, the last row and column -- of a partial tile --, the
first tile seam; the stride-2 convolution, where a position shows only the taps of one parity per axis, has the seam in all four parities), and every weight is a different integer code w[co, ci, ky, kx] = 1 + its flat index, so the output is a slice of the weight tensor
and a swapped tap or channel cannot cancel.  DoubleConv: either conv1 carries the codes (<= 1152) and conv2 is the centre-tap identity with slope 1, or
conv1 is the identity on channels 0 .. 7 and conv2 carries the codes (<= 576).  8x8: 4096 codes, more than fp16's 2048 integers, so two launches: the
codes 1 .. 2048 (zero elsewhere), then the codes above 2048 less 2048.
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# setting -> (precision mode, mc_stage, dc_valu, needs a context with weights loaded)
SETTINGS = {
    "fp32_s0": ("fp32", 0, 0, False),
    "fp32_s1": ("fp32", 1, 0, False),
    "bf16x3": ("bf16x3", 1, 0, False),
    "fp16": ("fp16", 1, 0, False),
    "bf16x2": ("bf16x2", 1, 0, False),
    "fp32_valu": ("fp32", 1, 2, False),     # every level-0 DoubleConv on hn_dcv.hip
    "fp32_asm": ("fp32", 1, 4, True),       # ... on hn_dca.hip (the default), whose zero page comes with hn_load_weights
}
FIVE = ("fp32_s0", "fp32_s1", "bf16x3", "fp16", "bf16x2")      # the exact legs run every case in these
FP32 = ("fp32_s0", "fp32_s1")
X16 = ("bf16x3", "fp16", "bf16x2")
SLOPES = (2.0, -0.5, 0.25, 0.0)                                 # 0: relu
ALL_CIN = (6, 8, 10, 16)
_STRIP = ((16, 128), (17, 130), (35, 194))                      # W >= 128: at least two tiles wide
_STRIP8 = ((8, 128), (9, 130), (19, 194))
_W256 = ((16, 256), (17, 258), (35, 322))
_every = lambda cins: {s: cins for s in FIVE}                   # noqa: E731


class Row:
    """One instance: op ('double_conv' | 'double_conv_smooth' | 'down' | 'up'), the planes (H, W) of the INPUT, the tile (rows, columns) in the
    coordinates the instance tiles (dc: the plane; down: the output; up: window rows x input columns), reached = {setting: input-channel counts}
    under which hn_module_route names the instance at every plane, extra = further settings the exact and random legs run (beside FIVE)."""

    def __init__(self, op, planes, tile, reached, batch3=1):
        self.op, self.planes, self.tile, self.reached, self.batch3 = op, planes, tile, reached, batch3

    @property
    def cins(self):
        return tuple(sorted({c for v in self.reached.values() for c in v}))

    def batch(self, plane):
        return 3 if plane == self.planes[self.batch3] else 2

    @property
    def big(self):
        """The plane with the most tiles and a part in both directions (the largest one): impulse, guard-word and NaN legs."""
        return max(self.planes, key=lambda p: p[0] * p[1])


TABLE = {
    "dc_asm": Row("double_conv", ((16, 256), (17, 260), (35, 324)), (16, 64), {"fp32_asm": (10, 16)}),          # W % 4 == 0; the input layer needs its 1e3
    "dc_valu": Row("double_conv", _W256, (16, 64), {"fp32_valu": (6, 10, 16), "fp32_asm": (6,)}),                 # (never the bottleneck)
    "k_dc_mfma_s": Row("double_conv", _STRIP + ((16, 256),), (16, 64), {"fp32_s0": ALL_CIN, "fp32_s1": (6, 8, 10), "fp32_valu": (8,), "fp32_asm": (8,)}),
    "k_dc_mfma_s_gen": Row("double_conv_smooth", _STRIP, (16, 64), _every(ALL_CIN)),
    "k_dc_mfma_s_ring": Row("double_conv", _STRIP + ((17, 258),), (16, 64), {"fp32_s1": (16,)}),
    "k_dc_mfma_p_32": Row("double_conv", ((8, 32), (9, 34), (19, 66), (8, 126)), (8, 32), _every(ALL_CIN)),
    "k_dc_mfma_p_16": Row("double_conv", ((2, 2), (8, 16), (9, 14), (19, 12)), (8, 16), _every(ALL_CIN)),          # W <= 16: one tile column
    "k_dc_mfma_64": Row("double_conv", ((16, 63), (17, 65), (35, 131), (18, 33)), (16, 64), _every(ALL_CIN)),       # odd W > 32; a 65-wide plane
    "k_dc_mfma_32": Row("double_conv", ((16, 31), (17, 17), (35, 27)), (16, 32), _every(ALL_CIN)),                  # odd 16 < W <= 32: one tile column
    "k_dc_mfma_16": Row("double_conv", ((1, 1), (5, 3), (16, 15), (35, 9)), (16, 16), _every(ALL_CIN)),
    "k_dc_x16_bf16x3": Row("double_conv", _STRIP8 + ((17, 258),), (8, 64), {"bf16x3": ALL_CIN}),
    "k_dc_x16_fp16": Row("double_conv", _STRIP + ((17, 258),), (16, 64), {"fp16": ALL_CIN}),
    "k_dc_x16_bf16x2": Row("double_conv", _STRIP + ((17, 258),), (16, 64), {"bf16x2": ALL_CIN}),
    # Wout > 64: 65 (Win % 4 == 2, an odd Wout above 64), 67, 131
    "down_64": Row("down", ((32, 130), (38, 134), (70, 262)), (16, 64), {"fp32_s0": (8,)}),
    "down_ring_64": Row("down", ((32, 130), (38, 134), (70, 262)), (16, 64), {"fp32_s1": (8,), "bf16x3": (8,)}),
    # 32 < Wout <= 64: 33 (Win 66), 35, two full tiles
    "down_32": Row("down", ((32, 66), (34, 70), (70, 128)), (16, 32), {"fp32_s0": (8,)}),
    "down_ring_32": Row("down", ((32, 66), (34, 70), (70, 128)), (16, 32), {"fp32_s1": (8,), "bf16x3": (8,)}),
    "down_16": Row("down", ((2, 2), (32, 32), (34, 34), (70, 54)), (16, 16), _every((8,))),
    "down_x16": Row("down", ((32, 128), (34, 130), (70, 166)), (16, 16), {"fp16": (8,), "bf16x2": (8,)}),
    # Win > 64: odd Hin and odd Win, Win = 65
    "up_2_11": Row("up", ((21, 65), (23, 67), (45, 98)), (22, 32), {"fp32_s0": (8,)}),
    "up_ring": Row("up", ((21, 65), (23, 67), (45, 98)), (22, 32), {"fp32_s1": (8,)}),
    "up_1_5": Row("up", ((1, 1), (19, 16), (20, 17), (41, 35)), (20, 16), {**_every((8,)), "fp32_valu": (8,)}),
    "up_x16": Row("up", ((19, 64), (20, 65), (41, 83)), (20, 16), {s: (8,) for s in X16}),
}
# the settings beside FIVE in which a row's exact and random legs also run (the instance is only reached there)
EXTRA = {"dc_asm": ("fp32_asm",), "dc_valu": ("fp32_valu", "fp32_asm")}
RING = ("k_dc_mfma_s_ring", "down_ring_64", "down_ring_32", "up_ring")       # 'mc_stage' 0 against 1: bit-equal on every plane
PAYLOAD = 0x7FC0BEEF


def header_routes():
    """{name: code} of enum hn_route in the header, names in lower case without the prefix."""
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    return {k.lower(): int(v) for k, v in re.findall(r"\bHN_ROUTE_([A-Z0-9_]+)\s*=\s*(\d+)", hdr)}


def out_shape(op, b, h, w):
    return (b, 8, h // 2, w // 2) if op == "down" else (b, 8, 2 * h, 2 * w) if op == "up" else (b, 8, h, w)


def tile_of(row, y, x):
    """Tile coordinates of OUTPUT element (y, x) in the instance's grid."""
    th, tw = row.tile
    if row.op == "up":      # y = 2 Y + 1 + py for window row Y = tile * th - 1 + r; x = 2 X + px
        return ((y + 1) // 2 // th, x // 2 // tw)
    return (y // th, x // tw)


def first_mismatch(row, got, want):
    """'' when equal bit for bit, else the first wrong (sample, channel, y, x), both values and the tile."""
    got, want = got.detach().cpu().double(), want.double()
    if got.shape == want.shape and torch.equal(got, want):
        return ""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = (got != want) | torch.isnan(got)
    s, c, y, x = (int(v) for v in bad.nonzero()[0])
    return (f"{int(bad.sum())} wrong, first at (sample {s}, channel {c}, y {y}, x {x}): got {got[s, c, y, x].item()!r}, want {want[s, c, y, x].item()!r}; "
            f"tile {tile_of(row, y, x)} of {row.tile}")


# ------------------------------------------------------------------------------------------ references
def dc_ref(x, w1, b1, slope, w2, b2, dtype=torch.float64):
    """DoubleConv with a piecewise-linear activation -> (mid after the activation, out)."""
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    h = F.conv2d(x, w1, b1, padding=1)
    mid = torch.where(h > 0, h, torch.tensor(float(slope), dtype=dtype) * h)
    return mid, F.conv2d(mid, w2, b2, padding=1)


def k8_ref(x, w, b, up, dtype=torch.float64):
    x, w, b = (t.to(dtype) for t in (x, w, b))
    return F.conv_transpose2d(x, w, b, stride=2, padding=3) if up else F.conv2d(x, w, b, stride=2, padding=3)


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _seed(inst, cin, plane, salt):
    return (sorted(TABLE).index(inst) * 1000003 + cin * 10007 + plane[0] * 401 + plane[1] + salt) % (2 ** 31)


def exact_case(inst, cin, plane):
    """Small-integer operands of one table case: dict(x, args (the weight tensors as Engine.double_conv / conv8x8 take them), act, slope, mid, want)."""
    row = TABLE[inst]
    g = torch.Generator().manual_seed(_seed(inst, cin, plane, 1))
    b, (h, w) = row.batch(plane), plane
    if row.op == "double_conv":
        slope = SLOPES[(cin + h + w) % 4]
        x, w1, b1, w2, b2 = _ints(g, (b, cin, h, w), 2), _ints(g, (8, cin, 3, 3), 2), _ints(g, (8,), 3), _ints(g, (8, 8, 3, 3), 2), _ints(g, (8,), 3)
        mid, want = dc_ref(x, w1, b1, slope, w2, b2)
        return dict(x=x, args=(w1, b1, slope, w2, b2), act="relu" if slope == 0.0 else "prelu", slope=slope, mid=mid, want=want)
    x, wt, bias = _ints(g, (b, 8, h, w), 4), _ints(g, (8, 8, 8, 8), 4), _ints(g, (8,), 3)
    return dict(x=x, args=(wt, bias), mid=None, want=k8_ref(x, wt, bias, row.op == "up"))


def impulse_positions(row, plane):
    """Input positions (y, x): a corner, the last row and column, the first tile seam (the row just past it, the column just before it)."""
    (h, w), (th, tw) = plane, row.tile
    sy, sx = (2 * th, 2 * tw - 1) if row.op == "down" else (th - 1, tw - 1) if row.op == "up" else (th, tw - 1)
    sy, sx = min(sy, h - 1), min(sx, w - 1)
    pos = [(0, 0), (h - 1, w - 1), (sy, sx)]
    if row.op == "down":     # stride 2: a position shows the taps of one parity per axis only, so the seam comes in all four parities
        pos += [(min(sy + dy, h - 1), min(sx + dx, w - 1)) for dy, dx in ((0, 1), (1, 0), (1, 1))]
    return tuple(pos)


def _codes(shape, lo=None):
    c = torch.arange(1, int(np.prod(shape)) + 1, dtype=torch.float32).reshape(shape)
    if lo is None:
        return c
    return torch.where(c <= 2048, c, torch.zeros(())) if lo else torch.where(c > 2048, c - 2048, torch.zeros(()))


def impulse_cases(inst, cin, plane):
    """The impulse launches of one table case: a list of dicts as exact_case returns.  Sample s has its 1 in channel s; as many rotations of the
    positions over the samples as there are positions, so that every (channel, position) pair occurs."""
    row = TABLE[inst]
    h, w = plane
    pos = impulse_positions(row, plane)
    eye = torch.zeros(8, 8, 3, 3)
    for c in range(8):
        eye[c, c, 1, 1] = 1.0
    zero8 = torch.zeros(8)
    out = []
    for rot in range(len(pos)):
        if row.op == "double_conv":
            x = torch.zeros(cin, cin, h, w)
            for s in range(cin):
                y, xx = pos[(s + rot) % len(pos)]
                x[s, s, y, xx] = 1.0
            m = min(cin, 8)
            eye1 = torch.zeros(8, cin, 3, 3)
            eye1[:, :m] = eye[:, :m]
            for w1, w2, xs in ((_codes((8, cin, 3, 3)), eye, x), (eye1, _codes((8, 8, 3, 3)), x[:m])):
                mid, want = dc_ref(xs, w1, zero8, 1.0, w2, zero8)
                out.append(dict(x=xs, args=(w1, zero8, 1.0, w2, zero8), act="prelu", slope=1.0, mid=mid, want=want))
        else:
            x = torch.zeros(8, 8, h, w)
            for s in range(8):
                y, xx = pos[(s + rot) % len(pos)]
                x[s, s, y, xx] = 1.0
            for lo in (True, False):
                wt = _codes((8, 8, 8, 8), lo)
                out.append(dict(x=x, args=(wt, zero8), mid=None, want=k8_ref(x, wt, zero8, row.op == "up")))
    return out


# ------------------------------------------------------------------------------------------ running a case on an Engine
def apply_setting(eng, setting, module_mc=1):
    prec, stage, valu, _ = SETTINGS[setting]
    eng.set_unet_precision(prec)
    eng.set_option("mc_stage", stage)
    eng.set_option("dc_valu", valu)
    eng.set_option("module_mc", module_mc)


def restore(eng):
    eng.set_unet_precision("fp32")
    for name, v in (("mc_stage", 1), ("dc_valu", 4), ("module_mc", 0)):
        eng.set_option(name, v)


def run(eng, row, case, dev):
    x = case["x"].to(dev)
    if row.op in ("double_conv", "double_conv_smooth"):
        return eng.double_conv(x, *case["args"], activation=case["act"])
    return eng.conv8x8(x, *case["args"], transposed=row.op == "up")
