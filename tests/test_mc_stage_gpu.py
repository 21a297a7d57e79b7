"""HN_OPT_MC_STAGE: the fp32 matrix-core 8x8 stride-2 convolutions and the decoder's strip DoubleConv with the input staging behind the MFMAs
(k_down_mfma_ring, k_up_mfma_ring, k_dc_mfma_s<.., RING> in hn_mfma.hip) against the kernels they replace.  Every accumulator receives the same MFMAs in the same order, so the contract is equality bit
for bit -- of one UNet evaluation and of three solver iterations, launched and captured -- plus the usual parity bar against the CPU oracle.

Sizes: 128^2 (level 0 on the 32-wide down tiles, every tile full), 144^2 (72- and 36-wide outputs: partial tiles in x and y on both tile
shapes, masked lanes, the dummy commit slot; 72 inputs wide for the transposed kernel) and 256^2 (the instances of the benchmark at levels 0 and 1
beside the deep-level launch and the side stream); for the decoder's strip kernel, which needs a level at least 128 wide, also 272^2 (level 1 is 136 wide:
partial tiles in x and y) and 512^2 (level 1 is four tiles wide)."""
import pytest
import torch

from golden_inputs import teacher_inputs
from oracle import helmnet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    yield s
    s.engine().set_option("mc_stage", 1)


def _inputs(solver, n, b):
    solver.set_domain_size(n, source_location=[n // 4, n // 2])
    ti = {k: torch.from_numpy(v).to(DEV) for k, v in teacher_inputs(n, b, seed=4100 + n + b).items()}
    k_sq, _ = solver.get_initials(ti["sos"])
    return ti, k_sq.contiguous(), solver._src()


def _finite_and_alive(tensors):
    return all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in tensors)


@pytest.mark.parametrize("n,b", [(128, 1), (128, 3), (144, 2), (256, 2), (272, 1), (512, 1)])
def test_unet_and_three_iterations_are_bit_identical(solver, n, b):
    ti, k_sq, src = _inputs(solver, n, b)
    e = solver.engine()
    in6 = torch.cat([ti["wf"], 1e3 * ti["res"], solver.sigmas.unsqueeze(0).repeat(b, 1, 1, 1)], 1).contiguous()
    got = {}
    for opt in (0, 1):
        e.set_option("mc_stage", opt)
        d, st_out = e.unet(in6, ti["states"].contiguous())
        wf, res, st = ti["wf"].clone(), ti["res"].clone(), ti["states"].clone()
        e.step(wf, res, st, k_sq, src, 3)
        torch.cuda.synchronize()
        e.check_async_errors()
        got[opt] = (d, st_out, wf, res, st)
    assert _finite_and_alive(got[0]) and not torch.equal(got[0][2], ti["wf"])
    for name, old, new in zip(("unet d", "unet states", "wavefield", "residual", "states"), got[0], got[1]):
        assert torch.equal(old, new), (name, float((old - new).abs().max()))


def test_captured_and_replayed_iterations_are_bit_identical(solver):
    """One iteration captured into a graph of the caller's and replayed twice, at 128^2 x 2, under either value of the option."""
    n, b = 128, 2
    ti, k_sq, src = _inputs(solver, n, b)
    e = solver.engine()
    got = {}
    for opt in (0, 1):
        e.set_option("mc_stage", opt)
        wf, res, st = ti["wf"].clone(), ti["res"].clone(), ti["states"].clone()
        e.step(wf, res, st, k_sq, src, 1)                    # eager: the first iteration
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream()
        with torch.cuda.stream(cap):
            with torch.cuda.graph(g, stream=cap):
                e.step(wf, res, st, k_sq, src, 1)
        g.replay()                                           # the second ...
        g.replay()                                           # ... and the third
        torch.cuda.synchronize()
        e.check_async_errors()
        got[opt] = (wf, res, st)
        del g
    e.set_option("mc_stage", 1)
    ref_wf, ref_res, ref_st = ti["wf"].clone(), ti["res"].clone(), ti["states"].clone()
    e.step(ref_wf, ref_res, ref_st, k_sq, src, 3)            # the same three iterations, launched
    torch.cuda.synchronize()
    assert _finite_and_alive(got[0])
    for name, old, new, ref in zip(("wavefield", "residual", "states"), got[0], got[1], (ref_wf, ref_res, ref_st)):
        assert torch.equal(old, new), (name, float((old - new).abs().max()))
        assert torch.equal(new, ref), (name, float((new - ref).abs().max()))


def test_single_step_matches_the_oracle_on_partial_tiles(solver, weights):
    """144^2 x 2 with the option at its default: wavefield, residual and hidden states within 1e-5 * max of the CPU oracle (the bar of the parity tests)."""
    n, b = 144, 2
    loc = [n // 4, n // 2]
    solver.engine().set_option("mc_stage", 1)
    solver.set_domain_size(n, source_location=loc)
    ti = {k: torch.from_numpy(v) for k, v in teacher_inputs(n, b, seed=4100 + n + b).items()}
    t = O.SpectralTables(n, 8, 2, 1.0)
    k_sq_o, _ = O.get_initials(ti["sos"], 1.0)
    want_wf, want_res, want_st = O.single_step(ti["wf"], k_sq_o, ti["res"], O.unflatten_states(ti["states"], n, 4), weights, O.point_source_map(n, loc, 10.0), t)
    g = {k: v.to(DEV) for k, v in ti.items()}
    k_sq, _ = solver.get_initials(g["sos"])
    solver.f.set_states(g["states"], flatten=True)
    wf2, res2 = solver.single_step(g["wf"], k_sq, g["res"])
    st2 = solver.f.get_states(flatten=True).cpu()
    errs = {
        "wf": ((wf2.cpu() - want_wf).abs().max() / want_wf.abs().max()).item(),
        "res": ((res2.cpu() - want_res).abs().max() / want_res.abs().max()).item(),
        "st": ((st2 - O.flatten_states(want_st)).abs().max() / O.flatten_states(want_st).abs().max()).item(),
    }
    print("MC_STAGE 144^2 x 2 single_step against the oracle:", errs)
    assert all(v <= 1e-5 for v in errs.values()), errs
