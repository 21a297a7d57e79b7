"""tests/mc_layers.py on the CPU: the table against the header's list of instances, and the preconditions under which the exact legs of
tests/test_mc_layers_gpu.py may demand bit equality -- asserted on the float64 REFERENCE of every case in the table; no kernel result enters."""
import pytest
import torch

import mc_layers as M
from helmnet_amd import _lib


def test_table_reaches_every_instance_the_header_lists():
    hdr = M.header_routes()
    assert hdr == _lib.HN_ROUTE and len(set(hdr.values())) == len(hdr)
    assert set(M.TABLE) == set(hdr) - {"direct"}
    assert _lib.HN_OPTION["module_mc"] == 20 and set(_lib.HN_ROUTE_OP) == {"double_conv", "down", "up", "double_conv_smooth"}
    for inst, row in M.TABLE.items():
        assert len(row.planes) >= 3 and row.reached and set(row.reached) <= set(M.SETTINGS), inst
        assert any(h != w for h, w in row.planes), inst
        assert sorted({row.batch(p) for p in row.planes}) == [2, 3], inst
        if row.op == "down":
            assert all(h % 2 == 0 and w % 2 == 0 for h, w in row.planes), inst
        assert all(h <= 70 and w <= 330 for h, w in row.planes), inst
    # the shapes the issue names
    assert {(1, 1), (5, 3)} <= set(M.TABLE["k_dc_mfma_16"].planes) and any(w == 65 for _, w in M.TABLE["k_dc_mfma_64"].planes)
    assert {66, 130} <= {w for k in ("down_32", "down_64") for _, w in M.TABLE[k].planes}
    assert any(w // 2 > 64 and (w // 2) % 2 for _, w in M.TABLE["down_64"].planes)
    for k in ("up_2_11", "up_1_5"):
        assert any(h % 2 for h, _ in M.TABLE[k].planes) and any(w % 2 for _, w in M.TABLE[k].planes), k
    assert any(w == 65 for _, w in M.TABLE["up_2_11"].planes)


def _is_int(t, scale=1.0):
    return bool((t * scale == (t * scale).round()).all())


def _one_operand_fits_8_bits(a, b):
    """The 2-part bf16 split drops (second part of a) x (second part of b): zero when either tensor holds integers of magnitude <= 256 only."""
    return any(_is_int(t) and float(t.abs().max()) <= 256 for t in (a, b))


EXACT_ROWS = [k for k, r in M.TABLE.items() if r.op != "double_conv_smooth"]


@pytest.mark.parametrize("inst", EXACT_ROWS)
def test_exact_cases_are_exact_in_every_format(inst):
    row = M.TABLE[inst]
    worst_mid, worst_out = 0.0, 0.0
    for plane in row.planes:
        for cin in row.cins:
            c = M.exact_case(inst, cin, plane)
            tensors = [c["x"]] + [t for t in c["args"] if isinstance(t, torch.Tensor)]
            assert all(_is_int(t) and float(t.abs().max()) <= 4 for t in tensors), (inst, cin, plane)
            assert c["x"].shape[0] == row.batch(plane) and tuple(c["want"].shape) == M.out_shape(row.op, c["x"].shape[0], *plane)
            assert float(c["want"].abs().max()) < 2 ** 24 and c["want"].abs().max() > 0
            if row.op == "double_conv":
                assert c["slope"] in M.SLOPES and _is_int(c["mid"], 4.0) and float(c["mid"].abs().max()) <= 512, (inst, cin, plane)
                assert torch.equal(c["mid"].half().double(), c["mid"])                    # the mid tensor is its own fp16 rounding
                mid32, out32 = M.dc_ref(c["x"], *c["args"], dtype=torch.float32)          # and the fp32 CPU composition is the float64 one
                assert torch.equal(mid32.double(), c["mid"]) and torch.equal(out32.double(), c["want"])
                worst_mid = max(worst_mid, float(c["mid"].abs().max()))
            else:
                assert torch.equal(M.k8_ref(c["x"], *c["args"], row.op == "up", dtype=torch.float32).double(), c["want"])
            worst_out = max(worst_out, float(c["want"].abs().max()))
    print(f"[{inst}] reference max |mid| {worst_mid:g}, max |out| {worst_out:g}")


@pytest.mark.parametrize("inst", EXACT_ROWS)
def test_impulse_cases_are_exact_and_show_every_weight_once(inst):
    row = M.TABLE[inst]
    plane, cin = row.big, row.cins[-1]
    h, w = plane
    pos = M.impulse_positions(row, plane)
    assert all(0 <= y < h and 0 <= x < w for y, x in pos) and pos[0] == (0, 0) and pos[1] == (h - 1, w - 1)
    cases = M.impulse_cases(inst, cin, plane)
    seen = set()
    for c in cases:
        x = c["x"]
        assert bool(((x == 0) | (x == 1)).all()) and bool((x.flatten(1).sum(1) == 1).all())       # one 1 per sample ...
        assert all(float(x[s, s].sum()) == 1 for s in range(x.shape[0]))                            # ... in channel s
        for s in range(x.shape[0]):
            y, xx = (int(v) for v in x[s, s].nonzero()[0])
            seen.add((s, pos.index((y, xx)) if (y, xx) in pos else -1))
        wts = [t for t in c["args"] if isinstance(t, torch.Tensor) and t.dim() == 4]
        for t in wts:      # all different where not zero (the identity of the other convolution is 0 / 1 and is not the tensor under test)
            nz = t[t != 0]
            assert _is_int(t) and float(t.abs().max()) <= 2048 and (nz.numel() == nz.unique().numel() or set(nz.tolist()) == {1.0}), inst
        assert _is_int(c["want"]) and float(c["want"].abs().max()) < 2 ** 24
        if c["mid"] is not None:
            assert _is_int(c["mid"]) and float(c["mid"].abs().max()) <= 2048
            assert _one_operand_fits_8_bits(x, c["args"][0]) and _one_operand_fits_8_bits(c["mid"], c["args"][3])
            # the output IS a weight slice: every non-zero output value is one of the codes
            codes = set(torch.cat([t.flatten() for t in wts]).tolist())
            assert set(c["want"].flatten().tolist()) <= codes | {0.0}
        else:
            assert set(c["want"].flatten().tolist()) <= set(wts[0].flatten().tolist()) | {0.0}
    assert -1 not in {p for _, p in seen}
    assert {p for s, p in seen if s == 0} == set(range(len(pos))) or len(pos) != len(set(pos))                 # every (channel, position) pair over the rotations
    if row.op != "double_conv":     # the two launches together carry all 4096 codes
        lo, hi = cases[0]["args"][0], cases[1]["args"][0]
        assert torch.equal(lo + torch.where(hi > 0, hi + 2048, torch.zeros(())), M._codes((8, 8, 8, 8)))
        shown = set().union(*(set(c["want"].flatten().tolist()) for c in cases[0::2])) | {v + 2048 for c in cases[1::2] for v in c["want"].flatten().tolist() if v}
        assert shown >= set(range(1, 4097)), (inst, len(shown))      # every tap of every channel pair appears in some output


def test_a_swapped_tap_or_channel_changes_an_impulse_reference():
    """What the impulse cases are for: exchanging two taps, or two input channels, of the coded weights changes the reference of a launch."""
    for inst in ("k_dc_mfma_p_32", "down_16", "up_1_5"):
        row = M.TABLE[inst]
        cases = M.impulse_cases(inst, row.cins[-1], row.big)
        for swap in ("tap", "channel"):
            changed = False
            for c in cases:
                wt = c["args"][0]
                w2 = wt.clone()
                if swap == "tap":
                    w2[..., 0, 0], w2[..., 0, 1] = wt[..., 0, 1], wt[..., 0, 0]
                else:
                    w2[:, 0], w2[:, 1] = wt[:, 1], wt[:, 0]
                args = (w2,) + tuple(c["args"][1:])
                other = M.dc_ref(c["x"], *args)[1] if row.op == "double_conv" else M.k8_ref(c["x"], *args, row.op == "up")
                changed = changed or not torch.equal(other, c["want"])
            assert changed, (inst, swap)


def test_first_mismatch_names_sample_channel_pixel_and_tile():
    row = M.TABLE["up_2_11"]
    want = torch.zeros(2, 8, 42, 130, dtype=torch.float64)
    got = want.float().clone()
    assert M.first_mismatch(row, got, want) == ""
    got[1, 3, 43 - 2, 129] = 1.0        # y = 41 = 2 * 20 + 1: window row 20, the last of the first block; x = 129: input column 64, the third tile
    msg = M.first_mismatch(row, got, want)
    assert "sample 1, channel 3, y 41, x 129" in msg and "tile (0, 2)" in msg, msg
    got[0, 0, 0, 0] = float("nan")
    assert "sample 0, channel 0, y 0, x 0" in M.first_mismatch(row, got, want)
    assert M.tile_of(M.TABLE["down_32"], 16, 33) == (1, 1) and M.tile_of(M.TABLE["k_dc_x16_bf16x3"], 8, 64) == (1, 1)
