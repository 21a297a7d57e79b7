"""The lean forms of the 256- and 512-point spectral kernels (hn_spectral.hip: complex multiplies and +-i rotations with the swap and the sign in
the operand modifiers of the packed instructions: the LeanOps policy) against the same kernel bodies instantiated on the plain C++ helpers
(HN_EXP_SPECTRAL_PLAIN 1: the PlainOps policy, kernels k_spec*_plain).  The lean forms claim the SAME products and the SAME fused multiply-adds: every comparison here is
torch.equal, on the probes of spectral_probes.py (noise, single modes along x and y, impulses) and on one solver iteration."""
import pytest
import torch

import spectral_probes as SP

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OPTIONS_256 = [(r, c) for r in (0, 1, 2) for c in (0, 1, 2)]   # (spectral_radix16, spectral_cols)
OPTIONS_512 = [0, 1]                                           # spectral_radix16
DEFAULTS = {"spectral_radix16": 1, "spectral_cols": 1, "spectral_plain": 0}


@pytest.fixture(scope="module")
def eng():
    from helmnet_amd.engine import Engine
    e = Engine(DEV)
    yield e
    e.close()


def _inputs(n, b):
    """b samples: the four probes, cycled; k_sq and one source per sample from their seeds."""
    u = SP.probe_batch(n)
    u = torch.cat([u] * (-(-b // len(SP.PROBES))))[:b].contiguous().to(DEV)
    return u, SP.seeded_k_sq(n, b, 5100 + n).to(DEV), SP.seeded_src(n, b, 7100 + n).to(DEV)


def _outputs(e, u, k_sq, src):
    """Laplacian (flags 1), residual with one shared source and with one source per sample (flags 3)."""
    return e.laplacian(u), e.residual(u, k_sq, src[:1].contiguous()), e.residual(u, k_sq, src)


@pytest.mark.parametrize("n,options", [(256, OPTIONS_256), (512, [(r, 1) for r in OPTIONS_512])])
@pytest.mark.parametrize("b", [1, 3])
def test_lean_kernels_give_the_bits_of_the_plain_ones(eng, n, options, b):
    """Batch 1 and a batch that is no multiple of the 8 XCDs the tile order deals samples over."""
    e = eng
    e.set_domain(n, *SP.DOMAIN)
    u, k_sq, src = _inputs(n, b)
    try:
        seen = set()
        for r, c in options:
            e.set_option("spectral_radix16", r)
            e.set_option("spectral_cols", c)
            out = {}
            for plain in (1, 0):
                e.set_option("spectral_plain", plain)
                out[plain] = _outputs(e, u, k_sq, src)
            for what, lean, ref in zip(("laplacian", "residual, one source", "residual, a source per sample"), out[0], out[1]):
                assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0, (r, c, what)
                assert torch.equal(lean, ref), (n, b, r, c, what, float((lean - ref).abs().max()))
            seen.add(out[0][1].cpu().numpy().tobytes())
        assert len(seen) == (3 if n == 256 else 2)      # the options do select different row kernels
    finally:
        for name, value in DEFAULTS.items():
            e.set_option(name, value)


@pytest.fixture(scope="module")
def solver():
    from helmnet_amd import IterativeSolver
    s = IterativeSolver.from_exported_weights()
    s.freeze()
    s.to(DEV)
    return s


def _step_args(solver, n, b):
    from helmnet_amd.phantoms import ring_sos_batch
    e = solver.engine()
    k_sq = ((1.0 / torch.from_numpy(ring_sos_batch(n, b, seed=31 + n))) ** 2).float().to(DEV).contiguous()
    src = solver._src()
    wf = torch.zeros(b, 2, n, n, device=DEV)
    res = e.residual(wf, k_sq, src)
    states = torch.zeros(b, 2, e.state_len, device=DEV)
    return [wf, res, states, k_sq, src]


@pytest.mark.parametrize("n,b", [(256, 2), (512, 1)])
def test_the_rmse_row_of_the_row_pass(solver, n, b):
    """The row pass sums the squares of what it stores into the RMSE history of hn_step.  Wavefield and residual after two iterations are
    bit-identical.  The RMSE row itself is NOT reproducible bit for bit, by either form: the 32 (256) / 64 (512) workgroups of a sample add
    their partial sums -- identical ones, the stored values being identical -- to one fp32 word with atomics, in the order they finish.  Two
    orders of a sum of m non-negative fp32 terms differ by at most 2 (m - 1) half-ulp roundings of partial sums not above the total: a relative
    2 (m - 1) 2^-24 on the sum, half of it on the root.  That is the bar ((m - 1) 2^-24: 1.8e-6 / 3.8e-6), with the sentinel rows around the table intact."""
    solver.set_domain_size(n, source_location=[n // 8 + 4, n // 2])
    e = solver.engine()
    got = {}
    try:
        for plain in (1, 0):
            e.set_option("spectral_plain", plain)
            args = _step_args(solver, n, b)
            guard = torch.full((2 + 8, b), -7.0, device=DEV)        # four sentinel rows each side (the table stays 16-byte aligned)
            e.step(*args, 2, rmse_hist=guard[4:-4])
            torch.cuda.synchronize()
            e.check_async_errors()
            got[plain] = (guard, args[0], args[1])
    finally:
        e.set_option("spectral_plain", 0)
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])
    blocks = n // 8
    lean, ref = got[0][0][4:-4].double(), got[1][0][4:-4].double()
    rel = float(((lean - ref).abs() / ref).max())
    print(f"SPEC n={n} rmse row, lean against plain: {rel:.2e} (bar {(blocks - 1) * 2.0 ** -24:.2e})")
    assert bool((ref > 0).all()) and rel <= (blocks - 1) * 2.0 ** -24
    for g in (got[0][0], got[1][0]):
        assert bool((g[:4] == -7.0).all()) and bool((g[-4:] == -7.0).all())


def test_one_solver_iteration_eager_and_captured_is_bit_identical(solver):
    """hn_step at 256^2, batch 2, default options: one iteration launched and one captured and replayed, lean against plain."""
    n, b = 256, 2
    solver.set_domain_size(n, source_location=[n // 8 + 4, n // 2])
    e = solver.engine()
    got = {}
    try:
        for plain in (1, 0):
            e.set_option("spectral_plain", plain)
            args = _step_args(solver, n, b)
            e.step(*args, 1)                                   # eager
            torch.cuda.synchronize()
            eager = [a.clone() for a in args[:3]]
            g = torch.cuda.CUDAGraph()
            cap = torch.cuda.Stream()
            with torch.cuda.stream(cap):
                with torch.cuda.graph(g, stream=cap):
                    e.step(*args, 1)
            g.replay()                                         # the second iteration
            torch.cuda.synchronize()
            e.check_async_errors()
            got[plain] = eager + [a.clone() for a in args[:3]]
            del g
    finally:
        e.set_option("spectral_plain", 0)
    assert all(bool(torch.isfinite(t).all()) for t in got[1]) and not torch.equal(got[1][0], got[1][3])
    for lean, ref in zip(got[0], got[1]):
        assert torch.equal(lean, ref)


# ------------------------------------------------------------------------------------------------ spectral_cols 3: k_spec8_cols_t
def _report(tag, got, want, bar):
    ratio = SP.errors(got, want) / bar[: got.shape[0]]
    print(f"SPEC {tag}: " + ", ".join(f"{nm} {float(r) * SP.BAR:.2e}" for nm, r in zip(SP.PROBES, ratio)) + f"  (bar {SP.BAR:.0e})")
    return float(ratio.max())


@pytest.fixture()
def eng_cols3(eng):
    eng.set_domain(256, *SP.DOMAIN)
    eng.set_option("spectral_cols", 3)
    yield eng
    eng.set_option("spectral_cols", DEFAULTS["spectral_cols"])


def test_cols3_matches_the_float64_oracle(eng_cols3):
    """Another factorisation than the radix-16 column kernels: its contract is the float64 oracle at the bar of every spectral route, for every
    probe, Laplacian and residual (one shared source; one source per sample on the first two probes)."""
    e, c = eng_cols3, SP.forward_case(256)
    u, k_sq = c["u"].to(DEV), c["k_sq"].to(DEV)
    lap = e.laplacian(u)
    res1 = e.residual(u, k_sq, c["src1"].to(DEV))
    res2 = e.residual(u[:2].contiguous(), k_sq[:2].contiguous(), c["src2"].to(DEV))
    worst = max(_report("n=256 cols=3 laplacian", lap, c["lap"], c["bar_lap"]), _report("n=256 cols=3 residual", res1, c["res1"], c["bar_res1"]),
                _report("n=256 cols=3 residual, a source per sample", res2, c["res2"], c["bar_res2"]))
    assert worst <= 1.0, worst * SP.BAR
    e.set_option("spectral_cols", 1)
    assert not torch.equal(e.laplacian(u), lap)      # the option does select another kernel


def test_cols3_a_sample_does_not_depend_on_its_batch(eng_cols3):
    """Batch 1, 3 and 33 (16 workgroups per sample, dealt over the 8 XCDs): the first and the last samples of the 33 on their own."""
    e = eng_cols3
    u, k_sq, src = _inputs(256, 33)
    want = e.residual(u, k_sq, src)
    for b in (1, 3):
        for first in (0, 33 - b):
            sl = slice(first, first + b)
            assert torch.equal(e.residual(u[sl].contiguous(), k_sq[sl].contiguous(), src[sl].contiguous()), want[sl]), (b, first)


def test_cols3_capture_and_replay(eng_cols3):
    e = eng_cols3
    u, k_sq, src = _inputs(256, 3)
    want = e.residual(u, k_sq, src)
    torch.cuda.synchronize()
    out = torch.full_like(u, float("nan"))
    g = torch.cuda.CUDAGraph()
    cap = torch.cuda.Stream()
    with torch.cuda.stream(cap):
        with torch.cuda.graph(g, stream=cap):
            out.copy_(e.residual(u, k_sq, src))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
