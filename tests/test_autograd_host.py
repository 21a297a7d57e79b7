"""CPU-only checks of the reverse-mode plumbing: the hn_step_vjp declaration and binding, and the pure-torch pieces of helmnet_amd.autograd."""
import os
import re
from ctypes import c_int, c_void_p

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_hn_step_vjp_and_lib_binds_it():
    from helmnet_amd import _lib
    hdr = open(os.path.join(REPO, "include", "helmnet_hip.h")).read()
    m = re.search(r"int hn_step_vjp\((.*?)\);", hdr, re.S)
    assert m, "hn_step_vjp is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 26
    res, args = _lib.SYMBOLS["hn_step_vjp"]
    assert res is c_int and len(args) == len(params)
    for p, a in zip(params, args):
        assert (a is c_int) == p.startswith("int "), (p, a)
        assert (a is c_void_p) == ("*" in p), (p, a)
    assert int(re.search(r"HN_VJP_CONTINUE\s*=\s*(\d+)", hdr).group(1)) == _lib.HN_VJP["continue"]
    assert int(re.search(r"HN_VJP_DEFER\s*=\s*(\d+)", hdr).group(1)) == _lib.HN_VJP["defer"]


def test_rmse_cotangent_matches_autograd():
    from helmnet_amd.autograd import rmse_cotangent
    g = torch.Generator().manual_seed(0)
    res = torch.randn(3, 2, 2, 8, 8, generator=g, dtype=torch.float64, requires_grad=True)
    rmse = res.pow(2).mean((2, 3, 4)).sqrt()                    # test_loss_function per (iteration, sample)
    g_rmse = torch.randn(3, 2, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(rmse, res, g_rmse)
    got = rmse_cotangent(g_rmse, res.detach(), rmse.detach())
    assert torch.allclose(got, want, rtol=1e-12, atol=0)


def _net(depth=4, act="prelu", state_depth=None):
    from helmnet_amd.unet import HybridNet
    torch.manual_seed(0)
    f = HybridNet(act, depth, 32, 8, 6, 2, depth if state_depth is None else state_depth)
    for p in f.parameters():
        torch.nn.init.normal_(p)
    return f


def test_weight_blob_is_pack_weights():
    from helmnet_amd.autograd import weight_blob
    from helmnet_amd.engine import pack_weights
    for depth, act, sd in ((4, "prelu", 4), (3, "relu", 2), (4, "gelu", 1)):
        f = _net(depth, act, sd)
        got = weight_blob(f).detach().numpy()
        want = pack_weights(dict(f.state_dict()), depth, act, sd)
        assert got.shape == want.shape and np.array_equal(got, want), (depth, act, sd)


def test_weight_blob_gradient_scatters_onto_the_parameters():
    """A known flat gradient on the blob lands on each parameter at its blob offset; padding and constant slopes get none."""
    from helmnet_amd.autograd import weight_blob
    from helmnet_amd.engine import weight_shapes
    from helmnet_amd.training import trainable_mask
    for depth, act, sd in ((4, "prelu", 4), (3, "relu", 2)):
        f = _net(depth, act, sd)
        blob = weight_blob(f)
        flat = torch.arange(blob.numel(), dtype=torch.float32) + 1.0
        blob.backward(flat)
        params = dict(f.named_parameters())
        mask = trainable_mask(depth, act, sd)
        seen, pos = 0, 0
        for name, shape in weight_shapes(depth).items():
            m = int(np.prod(shape))
            seg = flat[pos:pos + m].reshape(shape)
            if name in params:
                p = params[name]
                want = seg[:, :p.shape[1]] if p.shape != seg.shape else seg
                assert torch.equal(p.grad, want.reshape(p.shape)), name
                seen += p.numel()
                assert mask[pos:pos + m].reshape(shape)[(slice(None), slice(0, p.shape[1])) if p.shape != seg.shape else ...].all(), name
            else:
                assert not mask[pos:pos + m].any(), name
            pos += m
        assert seen == sum(p.numel() for p in f.parameters()) == int(mask.sum())
